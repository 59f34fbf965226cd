// The link between the two products of the lockstep when every column fits a resample of the rows of its own
// (include/fos_resample.h): a bootstrap sample, a subsample, bagging.
//
// Product 1 in its plain storing form leaves Z = A_panel Y of a row panel in rbuf16 (rows x 16 fp32, row-major), as for the
// pointwise link (pointwise_link.hpp), whose shape this kernel has: a lane takes one 16-byte quad of a row, grid-stride over
// the panel's rows x 4 quads, the fp64 loss sums go through DPP and LDS into q_part[wg][16] in a fixed order.  What it adds is
// the multiplicity c_ij in 0 .. 15 of row i in the resample that column j fits:
//
//     counts[i], one 8-byte word per row (little-endian): bits 4 j .. 4 j + 3 hold c_ij
//
// The four columns of a lane's quad are the 16-bit element idx of the same buffer viewed as uint16_t - the index of its quad -
// so the four lanes of a row read the row's word between them, 2 bytes each and 128 contiguous bytes per wave and trip.
//
// The loss is formed here for all five forms: product 1 never sees b, the weights or the counts.
//     Gram           R = z                                  (the operator A^T diag(w * c_j) A of the power iteration: no b, no sums)
//     squared        r = z - b,  R = r,  l = r^2 / 2
//     logistic       R = sigma(z) - b,  l = log(1 + e^z) - b z            (logistic_terms of product 1's own epilogue)
//     Huber, hinge   pointwise_terms (pointwise_link.hpp)
// In-bag (RESAMPLE_INBAG): R = (v w_i) c_ij and l = (l w_i) c_ij - the weight first, the count second, so that c = 1 gives the
// bits of the pointwise link and of product 1's weighted epilogue -, without WEIGHT R = v c_ij, l = l c_ij.  Out-of-bag
// (RESAMPLE_OOB): only the rows with c_ij = 0 count, each once (times w_i with WEIGHT); only the sums are wanted and R is not
// written.  There is no out-of-bag Gram form.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pointwise_link.hpp"

namespace fos {

constexpr int RL_THREADS = 256;
constexpr int RESAMPLE_GRAM = 0, RESAMPLE_SQUARED = 1, RESAMPLE_LOGISTIC = 2, RESAMPLE_HUBER = 3, RESAMPLE_SQUARED_HINGE = 4;
constexpr int RESAMPLE_INBAG = 0, RESAMPLE_OOB = 1;

// The pair (dl/dz, l) of one element in fp32 (the tests evaluate the same expressions in numpy fp32).
template <int LOSS>
__device__ __forceinline__ void resample_terms(float z, float b, float c, float half_c2, float* v, float* l) {
  if constexpr (LOSS == RESAMPLE_GRAM) {
    *v = z;
    *l = 0.f;
  } else if constexpr (LOSS == RESAMPLE_SQUARED) {
    const float r = z - b;
    *v = r;
    *l = __fmul_rn(0.5f * r, r);
  } else if constexpr (LOSS == RESAMPLE_LOGISTIC) {
    logistic_terms(z, b, v, l);
  } else if constexpr (LOSS == RESAMPLE_HUBER) {
    pointwise_terms<LINK_HUBER>(z, b, c, half_c2, v, l);
  } else {
    pointwise_terms<LINK_SQUARED_HINGE>(z, b, c, half_c2, v, l);
  }
}

// r16: the panel (rows x 16 fp32), a_i . y_j in, residuals out.  b[i]: the right-hand side or the label (unused by the Gram form,
// may be null there).  param: the Huber threshold.  nv: the active columns, 1 .. 16; columns >= nv are written as 0 and
// contribute 0.  counts16: the rows' words viewed as uint16_t (rows x 4 elements, 8-byte aligned).  row_weight: read with WEIGHT.
// q_part[wg][j] = the sum of l over this workgroup's rows for column j (fp64; fixed order, no atomics); not written by the Gram
// form (may be null).  stopped: the parking convention of product 1 (a set flag makes the launch a no-op).
// Rows >= rows are neither read nor written; the grid may be any size (grid-stride over the quads).
template <int LOSS, int MODE, bool WEIGHT>
__global__ __launch_bounds__(RL_THREADS) void resample_link_kernel(float* __restrict__ r16, int64_t rows, const float* __restrict__ b,
                                                                   float param, int nv, const float* __restrict__ row_weight,
                                                                   const uint16_t* __restrict__ counts16, double* __restrict__ q_part,
                                                                   const int* __restrict__ stopped) {
  static_assert(!(LOSS == RESAMPLE_GRAM && MODE == RESAMPLE_OOB), "the Gram form has no out-of-bag sums");
  if (stopped != nullptr && *stopped != 0) return;
  const int tid = threadIdx.x, quad = tid & 3;
  const float c = param, half_c2 = __fmul_rn(0.5f * c, c);
  bool live[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) live[k] = 4 * quad + k < nv;
  double qsum[4] = {0.0, 0.0, 0.0, 0.0};

  const int64_t total = rows * 4, stride = (int64_t)gridDim.x * RL_THREADS;
  for (int64_t idx = (int64_t)blockIdx.x * RL_THREADS + tid; idx < total; idx += stride) {
    const int64_t row = idx >> 2;
    f32x4* rp = reinterpret_cast<f32x4*>(r16) + idx;
    const f32x4 z4 = *rp;
    const unsigned c4 = counts16[idx];                 // this quad's four multiplicities, column 4 quad + k in bits 4 k .. 4 k + 3
    float bi = 0.f;
    if constexpr (LOSS != RESAMPLE_GRAM) bi = b[row];
    float w = 1.f;
    if constexpr (WEIGHT) w = row_weight[row];
    f32x4 out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v, l;
      resample_terms<LOSS>(z4[k], bi, c, half_c2, &v, &l);
      if constexpr (WEIGHT) { v *= w; l *= w; }
      const unsigned ck = (c4 >> (4 * k)) & 0xfu;
      bool keep = live[k];
      if constexpr (MODE == RESAMPLE_OOB) {
        keep = keep && ck == 0u;
      } else {
        const float cf = (float)ck;
        v *= cf;
        l *= cf;
      }
      v = keep ? v : 0.f;
      l = keep ? l : 0.f;
      if constexpr (LOSS != RESAMPLE_GRAM) qsum[k] += (double)l;
      out[k] = v;
    }
    if constexpr (MODE != RESAMPLE_OOB) *rp = out;
  }

  if constexpr (LOSS != RESAMPLE_GRAM) {
    // lanes of equal quad within a 16-lane row (DPP row_shr 4, 8: lanes 12 .. 15 hold the totals) -> LDS -> the workgroup's row
    // of q_part, every sum in a fixed order
    __shared__ double red[RL_THREADS / 16][BT_NV];    // [16-lane row of the workgroup][column]
#pragma unroll
    for (int k = 0; k < 4; ++k) qsum[k] += dpp_fetch<0x114, 0xF>(qsum[k]);     // row_shr:4
#pragma unroll
    for (int k = 0; k < 4; ++k) qsum[k] += dpp_fetch<0x118, 0xF>(qsum[k]);     // row_shr:8
    if ((tid & 15) >= 12) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[tid >> 4][4 * quad + k] = qsum[k];
    }
    __syncthreads();
    if (tid < BT_NV) {
      double v = 0.0;
#pragma unroll
      for (int g = 0; g < RL_THREADS / 16; ++g) v += red[g][tid];
      q_part[(int64_t)blockIdx.x * BT_NV + tid] = v;
    }
  }
}

}  // namespace fos
