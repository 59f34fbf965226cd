// fp64-accumulating fg for up to 16 points at once, on the fp64 matrix cores (fos_gemv_pair_dd_multi):
//   G[:, j] = A^T (A X[:, j] - B[:, j]) + alpha2 X[:, j],   rr[j] = ||A X[:, j] - B[:, j]||^2,   every sum in fp64.
// The arithmetic of fos_gemv_pair_dd for each column: A (fp32 / bf16 as stored) is widened to fp64 exactly, X is never
// rounded, only the order of the sums differs.  The pair has the shape of the fp32 lockstep pair (gram_batch.hpp) with
// fp64 data throughout, over row panels:
//   product 1  R[P x 16] = A_panel X - B16_panel    residual_dd_mfma_kernel   (A from HBM)
//   product 2  G[16 x n] (+)= R^T A_panel           gram_dd_mfma_kernel       (the panel again)
// Both on v_mfma_f64_16x16x4_f64: A/B one f64 per lane as in the f32 16x16x4 form (lane l: A[l&15][k = l>>4],
// B[k = l>>4][l&15]), C/D col = lane&15, row = (lane>>4) + 4*reg.  Tiles of A (64 x 64 elements) go through LDS as
// they are stored and are widened to fp64 when the operands are built; R, the slabs and their reduction are fp64.
// Columns of X beyond nv (or of a finished fit) are zero in the staged block: the pass costs the same, their result is
// not used.
#pragma once
#include "batch_trial.hpp"

namespace fos {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int DM_ROWS = 64, DM_COLS = 64, DM_THREADS = 256;
constexpr int DM_RSTRIDE = BT_NV + 4;          // doubles: rows 4 apart land 128 bytes apart (two LDS passes per read)
constexpr int DM_X_TILE = DM_COLS * BT_NV;     // doubles of the staged X block per column tile (Xp layout, xp_index)

// A tile in LDS as stored: 32-bit words, rows padded by 4 words (fp32: 4q rows apart -> 16 banks apart; bf16: 16 banks).
template <typename T> struct DmTile;
template <> struct DmTile<float> {
  static constexpr int EPC = 4, WORDS = DM_COLS + 4;
  __device__ static inline double at(const unsigned* row, int col) { return (double)__uint_as_float(row[col]); }
  __device__ static inline void four(const unsigned* row, int col, double (&o)[4]) {      // col % 4 == 0
    const u32x4 v = *reinterpret_cast<const u32x4*>(row + col);
    o[0] = __uint_as_float(v.x); o[1] = __uint_as_float(v.y); o[2] = __uint_as_float(v.z); o[3] = __uint_as_float(v.w);
  }
};
template <> struct DmTile<bf16_t> {
  static constexpr int EPC = 8, WORDS = DM_COLS / 2 + 4;
  __device__ static inline double at(const unsigned* row, int col) {
    return (double)bf16_to_f32(reinterpret_cast<const unsigned short*>(row)[col]);
  }
  __device__ static inline void four(const unsigned* row, int col, double (&o)[4]) {      // col % 4 == 0
    const u32x2 v = *reinterpret_cast<const u32x2*>(row + col / 2);
    o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
    o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  }
};

// Product 1: rout[row][16] = A_row . Xd_j - b16[row][j] (fp64) and q_part[wg][j] = sum over the workgroup's rows of its
// square.  Requirements (host-checked): the aligned layout (n % EPC == 0, lda % EPC == 0, A 16-byte aligned), Xd zero-padded
// to a multiple of 64 columns.  A workgroup takes groups of 64 rows (wave w: rows 16w..16w+15) and walks the row's column
// tiles; two register sets keep two tiles in flight (the straight-line pair loop of residual_batch_mfma_kernel).
template <typename T>
__global__ __launch_bounds__(DM_THREADS) void residual_dd_mfma_kernel(const T* __restrict__ A, int64_t lda,
                                                                     const float* __restrict__ b16, int64_t m, int n,
                                                                     const double* __restrict__ xd, int64_t groups_per_wg,
                                                                     double* __restrict__ q_part, double* __restrict__ rout) {
  using Tl = DmTile<T>;
  constexpr int CPR = DM_COLS / Tl::EPC;                    // 16-byte chunks per tile row
  constexpr int A_LOADS = DM_ROWS * CPR / DM_THREADS;       // 4 (fp32) / 2 (bf16)
  constexpr int X_LOADS = DM_X_TILE / 2 / DM_THREADS;       // 16-byte chunks of the X tile per thread: 2
  __shared__ __attribute__((aligned(16))) unsigned a_s[2][DM_ROWS][Tl::WORDS];
  __shared__ __attribute__((aligned(16))) double x_s[2][DM_X_TILE];
  __shared__ double wsum[4][BT_NV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ngroups = (m + DM_ROWS - 1) / DM_ROWS;
  const int64_t g_lo = (int64_t)blockIdx.x * groups_per_wg;
  int64_t g_hi = g_lo + groups_per_wg;
  if (g_hi > ngroups) g_hi = ngroups;
  const int ktiles = (n + DM_COLS - 1) / DM_COLS;
  const int64_t ntiles = (g_hi > g_lo ? (g_hi - g_lo) : 0) * ktiles;

  u32x4 areg[2][A_LOADS];
  f64x2 xreg[2][X_LOADS];
  auto load_tile = [&](int set, int64_t t) {
    const int64_t row0 = (g_lo + t / ktiles) * DM_ROWS;
    const int kt = (int)(t % ktiles);
    const int col0 = kt * DM_COLS;
#pragma unroll
    for (int u = 0; u < A_LOADS; ++u) {
      const int f = u * DM_THREADS + tid;
      int64_t row = row0 + f / CPR;
      int col = col0 + Tl::EPC * (f % CPR);
      if (row >= m) row = m - 1;                   // clamped rows are not stored
      if (col >= n) col = n - Tl::EPC;             // clamped columns meet zero rows of Xd
      areg[set][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(A + row * lda + col));
    }
#pragma unroll
    for (int u = 0; u < X_LOADS; ++u)
      xreg[set][u] = *reinterpret_cast<const f64x2*>(xd + (int64_t)kt * DM_X_TILE + 2 * (u * DM_THREADS + tid));
  };
  auto store_tile = [&](int set, int buf) {
#pragma unroll
    for (int u = 0; u < A_LOADS; ++u) {
      const int f = u * DM_THREADS + tid;
      *reinterpret_cast<u32x4*>(&a_s[buf][f / CPR][4 * (f % CPR)]) = areg[set][u];
    }
#pragma unroll
    for (int u = 0; u < X_LOADS; ++u) *reinterpret_cast<f64x2*>(&x_s[buf][2 * (u * DM_THREADS + tid)]) = xreg[set][u];
  };
  f64x4 acc = {0.0, 0.0, 0.0, 0.0}, acc_odd = {0.0, 0.0, 0.0, 0.0};
  double qsum = 0.0;                                // this lane's vector j = lane & 15
  const int q = lane >> 4, i = lane & 15;
  auto compute_tile = [&](int buf, int64_t t) {
    const unsigned* arow = a_s[buf][16 * wave + i];
#pragma unroll
    for (int sub = 0; sub < DM_COLS / 16; ++sub) {
      // lane (q, i): A[row 16w + i][col 16 sub + 4q + c] and X[col 16 sub + 4q + c][vector i] for MFMA step c
      double a[4];
      Tl::four(arow, 16 * sub + 4 * q, a);
      const f64x2 x01 = *reinterpret_cast<const f64x2*>(&x_s[buf][(sub * 4 + q) * 64 + i * 4]);
      const f64x2 x23 = *reinterpret_cast<const f64x2*>(&x_s[buf][(sub * 4 + q) * 64 + i * 4 + 2]);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], x01.x, acc, 0, 0, 0);
      acc_odd = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], x01.y, acc_odd, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[2], x23.x, acc, 0, 0, 0);
      acc_odd = __builtin_amdgcn_mfma_f64_16x16x4f64(a[3], x23.y, acc_odd, 0, 0, 0);
    }
    if ((t + 1) % ktiles == 0) {
      // row group complete: D[row = (lane>>4) + 4 reg][vector = lane&15]
      acc += acc_odd;
      const int64_t row0 = (g_lo + t / ktiles) * DM_ROWS + 16 * wave + q;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = row0 + 4 * r;
        if (row < m) {
          const double v = acc[r] - (double)b16[row * BT_NV + i];
          qsum += v * v;
          rout[row * BT_NV + i] = v;               // 16 lanes: one 128-byte row of R
        }
      }
      acc = f64x4{0.0, 0.0, 0.0, 0.0};
      acc_odd = f64x4{0.0, 0.0, 0.0, 0.0};
    }
  };
  if (ntiles > 0) {
    const int64_t last = ntiles - 1;
    auto clampt = [&](int64_t t) { return t < last ? t : last; };
    load_tile(0, 0);
    store_tile(0, 0);
    load_tile(1, clampt(1));
    __syncthreads();
    int64_t t = 0;
    for (; t + 2 <= ntiles; t += 2) {
      load_tile(0, clampt(t + 2));
      compute_tile(0, t);
      store_tile(1, 1);
      __syncthreads();
      load_tile(1, clampt(t + 3));
      compute_tile(1, t + 1);
      store_tile(0, 0);
      __syncthreads();
    }
    if (t < ntiles) compute_tile(0, t);
  }
  qsum += __shfl_xor(qsum, 16, 64);
  qsum += __shfl_xor(qsum, 32, 64);
  if (lane < BT_NV) wsum[wave][lane] = qsum;
  __syncthreads();
  if (tid < BT_NV) q_part[(int64_t)blockIdx.x * BT_NV + tid] = (wsum[0][tid] + wsum[1][tid]) + (wsum[2][tid] + wsum[3][tid]);
}

// Product 2: slabs[split][j][col] (+)= sum over the split's rows of R[row][j] * A[row][col].  A workgroup owns a 64-column
// strip of a row split (wave w: columns 16w..16w+15) and walks it in 64-row tiles.  Per 16 rows four MFMAs, step c taking
// rows 16 ks + 4q + c (lane (q, i): R[row][vector i] as the A operand, A[row][column 16w + i] as the B operand).
// Rows past the split meet zero rows of R; columns past n are not stored.  ACCUM: later panels add to the slabs.
template <typename T, bool ACCUM>
__global__ __launch_bounds__(DM_THREADS) void gram_dd_mfma_kernel(const T* __restrict__ A, int64_t lda, int64_t m, int n,
                                                                 const double* __restrict__ R, int64_t rows_per_split,
                                                                 double* __restrict__ slabs, int64_t n_stride) {
  using Tl = DmTile<T>;
  constexpr int CPR = DM_COLS / Tl::EPC;
  constexpr int A_LOADS = DM_ROWS * CPR / DM_THREADS;
  constexpr int R_LOADS = DM_ROWS * BT_NV / 2 / DM_THREADS;       // 16-byte chunks of the R tile per thread: 2
  __shared__ __attribute__((aligned(16))) unsigned a_s[2][DM_ROWS][Tl::WORDS];
  __shared__ __attribute__((aligned(16))) double r_s[2][DM_ROWS][DM_RSTRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col0 = blockIdx.x * DM_COLS;
  const int64_t row_lo = (int64_t)blockIdx.y * rows_per_split;
  int64_t row_hi = row_lo + rows_per_split;
  if (row_hi > m) row_hi = m;
  const int64_t ntiles = row_hi > row_lo ? (row_hi - row_lo + DM_ROWS - 1) / DM_ROWS : 0;

  u32x4 areg[2][A_LOADS];
  f64x2 rreg[2][R_LOADS];
  auto load_tile = [&](int set, int64_t t) {
    const int64_t row0 = row_lo + t * DM_ROWS;
#pragma unroll
    for (int u = 0; u < A_LOADS; ++u) {
      const int f = u * DM_THREADS + tid;
      int64_t row = row0 + f / CPR;
      int col = col0 + Tl::EPC * (f % CPR);
      if (row >= row_hi) row = row_hi - 1;         // clamped rows meet zero rows of R
      if (col >= n) col = n - Tl::EPC;             // clamped columns are not stored
      areg[set][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(A + row * lda + col));
    }
#pragma unroll
    for (int u = 0; u < R_LOADS; ++u) {
      const int f = u * DM_THREADS + tid;          // 64 rows x 8 chunks of two doubles
      int64_t rrow = row0 + f / 8;
      const bool in = rrow < row_hi;
      if (!in) rrow = row_hi - 1;
      const f64x2 rv = *reinterpret_cast<const f64x2*>(R + rrow * BT_NV + 2 * (f % 8));
      rreg[set][u] = in ? rv : f64x2{0.0, 0.0};
    }
  };
  auto store_tile = [&](int set, int buf) {
#pragma unroll
    for (int u = 0; u < A_LOADS; ++u) {
      const int f = u * DM_THREADS + tid;
      *reinterpret_cast<u32x4*>(&a_s[buf][f / CPR][4 * (f % CPR)]) = areg[set][u];
    }
#pragma unroll
    for (int u = 0; u < R_LOADS; ++u) {
      const int f = u * DM_THREADS + tid;
      *reinterpret_cast<f64x2*>(&r_s[buf][f / 8][2 * (f % 8)]) = rreg[set][u];
    }
  };
  f64x4 acc = {0.0, 0.0, 0.0, 0.0}, acc_odd = {0.0, 0.0, 0.0, 0.0};
  const int q = lane >> 4, i = lane & 15;
  auto compute_tile = [&](int buf) {
#pragma unroll
    for (int ks = 0; ks < DM_ROWS / 16; ++ks) {
      const int r0 = 16 * ks + 4 * q;
#pragma unroll
      for (int c = 0; c < 4; c += 2) {
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(r_s[buf][r0 + c][i], Tl::at(a_s[buf][r0 + c], 16 * wave + i), acc, 0, 0, 0);
        acc_odd = __builtin_amdgcn_mfma_f64_16x16x4f64(r_s[buf][r0 + c + 1][i], Tl::at(a_s[buf][r0 + c + 1], 16 * wave + i),
                                                       acc_odd, 0, 0, 0);
      }
    }
  };
  if (ntiles > 0) {
    const int64_t last = ntiles - 1;
    auto clampt = [&](int64_t t) { return t < last ? t : last; };
    load_tile(0, 0);
    store_tile(0, 0);
    load_tile(1, clampt(1));
    __syncthreads();
    int64_t t = 0;
    for (; t + 2 <= ntiles; t += 2) {
      load_tile(0, clampt(t + 2));
      compute_tile(0);
      store_tile(1, 1);
      __syncthreads();
      load_tile(1, clampt(t + 3));
      compute_tile(1);
      store_tile(0, 0);
      __syncthreads();
    }
    if (t < ntiles) compute_tile(0);
  }
  acc += acc_odd;
  const int col = col0 + 16 * wave + i;
  if (col < n) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {                  // D[vector = (lane>>4) + 4 reg][column = lane&15]
      double* dst = slabs + ((int64_t)blockIdx.y * BT_NV + q + 4 * r) * n_stride + col;
      if constexpr (ACCUM) *dst += acc[r];
      else *dst = acc[r];
    }
  }
}

// Pointers of the columns of one multi-point pass.  col[y] = the column that blockIdx.y serves (finished fits are left out).
struct DdMultiCols {
  const double* x[BT_NV];           // the points (n doubles each)
  double* g[BT_NV];                 // their gradients
  double* rr[BT_NV];                // ||r||^2 (one double each)
  int col[BT_NV];
};

// The points -> the zero-padded block Xd (Xp layout in doubles).  Columns not in `live` (bit j) are zero.
static __global__ __launch_bounds__(256) void xd_pack_kernel(DdMultiCols c, unsigned live, int n, int n_pad,
                                                            double* __restrict__ xd) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < (int64_t)n_pad * BT_NV; e += (int64_t)gridDim.x * 256) {
    const int col = (int)(e / BT_NV), j = (int)(e % BT_NV);
    xd[xp_index(col, j)] = (col < n && ((live >> j) & 1u)) ? c.x[j][col] : 0.0;
  }
}

// G_j = sum of the slab sets (fixed order) + alpha2 * x_j; block x = 0 also folds rr_j from the product-1 partials.
static __global__ __launch_bounds__(256) void pair_dd_multi_finish_kernel(const double* __restrict__ slabs, int splits, int n,
                                                                         const double* __restrict__ q_part, int nparts,
                                                                         double alpha2, DdMultiCols c) {
  const int j = c.col[blockIdx.y];
  for (int col = blockIdx.x * 256 + threadIdx.x; col < n; col += gridDim.x * 256) {
    double s = 0.0;
    for (int sp = 0; sp < splits; ++sp) s += slabs[((int64_t)sp * BT_NV + j) * n + col];
    c.g[j][col] = s + alpha2 * c.x[j][col];
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    double s = 0.0;
    for (int w = threadIdx.x; w < nparts; w += 64) s += q_part[(int64_t)w * BT_NV + j];
    s = wave_sum(s);
    if (threadIdx.x == 0) *c.rr[j] = s;
  }
}

}  // namespace fos
