// The link between the two products of the lockstep for a pointwise loss: Huber and the squared hinge.
//
// Product 1 in its plain storing form leaves Z = A_panel Y of a row panel in rbuf16 (rows x 16 fp32, row-major).  Both losses
// are pointwise: column j's residual entry depends on its own z = a_i . y_j and on b_i alone,
//
//     Huber, threshold c:  r = z - b      R = clip(r, -c, c)        l = r^2 / 2 (|r| <= c),  c |r| - c^2 / 2 (otherwise)
//     squared hinge:       u = max(0, 1 - b z)   R = -b u           l = u^2 / 2                      (labels b = -1 / +1)
//
// so the panel is rewritten in place and product 2 follows, as on a multinomial problem (softmax_link.hpp).  |dR/dz| <= 1 for
// both: the Lipschitz constant is the squared loss's and the lockstep keeps its fixed step.
//
// No lane needs a whole row here, so a lane takes one 16-byte quad of a row: element idx of the panel's rows x 4 quads is row
// idx >> 2, quad idx & 3.  A wave then loads and stores 1 KiB of contiguous memory per trip (global_load / _store_dwordx4,
// fully coalesced); the four lanes of a row read the same b, weight and fold id.  The grid stride is a multiple of 4, so a
// lane's quad - its four columns, their held ids, whether they are below nv - is fixed for the whole launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batch_trial.hpp"

namespace fos {

constexpr int PL_THREADS = 256;
constexpr int LINK_HUBER = 0, LINK_SQUARED_HINGE = 1;

// The pair (dl/dz, l) of one element, in fp32 and in this order (the tests evaluate the same expressions in numpy fp32).
// The products that an addition follows are rounded on their own (no contraction into an fma).
template <int LINK>
__device__ __forceinline__ void pointwise_terms(float z, float b, float c, float half_c2, float* v, float* l) {
  if constexpr (LINK == LINK_HUBER) {
    const float r = z - b;
    const float a = fabsf(r);
    *v = fminf(fmaxf(r, -c), c);
    *l = a <= c ? __fmul_rn(0.5f * r, r) : __fsub_rn(__fmul_rn(c, a), half_c2);
  } else {
    const float u = fmaxf(0.f, __fsub_rn(1.f, __fmul_rn(b, z)));
    *v = -b * u;
    *l = __fmul_rn(0.5f * u, u);
  }
}

// r16: the panel (rows x 16 fp32), a_i . y_j in, residuals out.  b[i]: the right-hand side (Huber) or the label -1 / +1
// (squared hinge).  param: the Huber threshold c > 0 (unused by the hinge).  nv: the active columns, 1 .. 16; columns >= nv are
// written as 0 and contribute 0.
// WEIGHT: R and l are multiplied by row_weight[i].  FOLD: the mask of K-fold cross-validation with the semantics of fold_mask
// (batch_trial.hpp), column j against fold_held_of(held, j); FOLD_TRAIN zeroes R and l on the rows column j holds out, FOLD_HELD
// everywhere else.  In the FOLD_HELD form only the sums are wanted and R is not written.
// q_part[wg][j] = the sum of l over this workgroup's rows for column j (fp64; fixed order, no atomics).
// stopped: the parking convention of product 1 (a set flag makes the launch a no-op).
// Rows >= rows are neither read nor written; the grid may be any size (grid-stride over the quads).
template <int LINK, int FOLD, bool WEIGHT>
__global__ __launch_bounds__(PL_THREADS) void pointwise_link_kernel(float* __restrict__ r16, int64_t rows,
                                                                    const float* __restrict__ b, float param, int nv,
                                                                    const float* __restrict__ row_weight,
                                                                    const uint8_t* __restrict__ fold_of_row, FoldHeld held,
                                                                    double* __restrict__ q_part,
                                                                    const int* __restrict__ stopped) {
  if (stopped != nullptr && *stopped != 0) return;
  __shared__ double red[PL_THREADS / 16][BT_NV];    // [16-lane row of the workgroup][column]
  const int tid = threadIdx.x, quad = tid & 3;
  const float c = param, half_c2 = __fmul_rn(0.5f * c, c);
  // this lane's four columns: whether they are active and the fold each holds out
  bool live[4];
  unsigned held_id[4];
  {
    unsigned w[4];
    __builtin_memcpy(w, &held, sizeof(w));
    const unsigned ws = quad == 0 ? w[0] : quad == 1 ? w[1] : quad == 2 ? w[2] : w[3];    // fold_held_of(held, 4 quad + k)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      live[k] = 4 * quad + k < nv;
      held_id[k] = (ws >> (8 * k)) & 0xffu;
    }
  }
  double qsum[4] = {0.0, 0.0, 0.0, 0.0};

  const int64_t total = rows * 4, stride = (int64_t)gridDim.x * PL_THREADS;
  for (int64_t idx = (int64_t)blockIdx.x * PL_THREADS + tid; idx < total; idx += stride) {
    const int64_t row = idx >> 2;
    f32x4* rp = reinterpret_cast<f32x4*>(r16) + idx;
    const f32x4 z4 = *rp;
    const float bi = b[row];
    float w = 1.f;
    if constexpr (WEIGHT) w = row_weight[row];
    unsigned fold_id = 0u;
    if constexpr (FOLD != FOLD_OFF) fold_id = fold_of_row[row];
    f32x4 out;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float v, l;
      pointwise_terms<LINK>(z4[k], bi, c, half_c2, &v, &l);
      if constexpr (WEIGHT) { v *= w; l *= w; }
      bool keep = live[k];
      if constexpr (FOLD != FOLD_OFF) {
        const bool is_held = fold_id == held_id[k];
        keep = keep && (FOLD == FOLD_TRAIN ? !is_held : is_held);
      }
      v = keep ? v : 0.f;
      l = keep ? l : 0.f;
      qsum[k] += (double)l;
      out[k] = v;
    }
    if constexpr (FOLD != FOLD_HELD) *rp = out;
  }

  // lanes of equal quad within a 16-lane row (DPP row_shr 4, 8: lanes 12 .. 15 hold the totals) -> LDS -> the workgroup's row
  // of q_part, every sum in a fixed order
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
    for (int g = 0; g < PL_THREADS / 16; ++g) v += red[g][tid];
    q_part[(int64_t)blockIdx.x * BT_NV + tid] = v;
  }
}

}  // namespace fos
