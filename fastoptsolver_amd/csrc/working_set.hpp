// Working-set solve of a sparse path (include/fos_working_set.h): the column gather and the KKT scan.  The lockstep runs on the
// gathered matrix as on any other fos_problem; these two kernels and fos_gradient_batch (existing launches) are all the outer
// loop of fastoptsolver_amd/working_set.py needs from the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_trial.hpp"

namespace fos {

// ---- column gather ------------------------------------------------------------------------------------------------------------
// A_ws[i][c] = A[i][idx[c]] (c < n_ws), 0 (n_ws <= c < n_ws_pad).  The per-lane form: one lane per working-set column, a
// workgroup takes a panel of whole rows, idx sits in LDS for the whole panel (chunks of WS_IDX_CHUNK columns), WS_ROWS rows are
// in flight per lane.  idx is sorted, so the lanes of a wave walk a row in address order and neighbouring lanes share or
// neighbour 128-byte lines: the kernel requests the lines of a row that hold a gathered column, each once per chunk, in order -
// at most the row itself.  The dense-read form (whole rows through LDS, picked from there) always fetches all of A; at the
// line granularity of the memory system the two meet once about every line holds a gathered column (n_ws >= n / 32 in fp32,
// n / 64 in bf16, for scattered columns) and the per-lane form fetches less below that, with no LDS traffic for the data and no
// second pass over it.  Rows are never split between workgroups, so no line is requested by two of them.  Loads are non-temporal
// (A is streamed once), the stores of a wave are 64 consecutive elements.  Measured once (tools/bench_working_set.py,
// profiles/working_set/README.md): 1.33 x the time of a read-only pass over A at 65536 x 8192 fp32 with 428 columns, 0.65 x at
// 131072 x 16384 bf16 with 136, 4.9 x at 262144 x 256, where 128 columns fill a quarter of the workgroup.  An idx entry outside
// 0..n-1 (the caller's error) reads nothing and stores 0.
// Resources (gfx950, -O3): 40 VGPRs for either element size, 32 KiB of LDS, no scratch, no atomics.
constexpr int WS_THREADS = 512;
constexpr int WS_IDX_CHUNK = 8192;
constexpr int WS_ROWS = 4;

template <int ESZ> struct ws_elem;
template <> struct ws_elem<4> { using type = uint32_t; };
template <> struct ws_elem<2> { using type = uint16_t; };

template <int ESZ>
static __global__ __launch_bounds__(WS_THREADS) void gather_columns_kernel(const void* __restrict__ A_, int64_t lda, int64_t m, int n,
                                                                           const int32_t* __restrict__ idx, int n_ws, int n_ws_pad,
                                                                           void* __restrict__ out_, int64_t lda_ws,
                                                                           int64_t rows_per_wg) {
  using T = typename ws_elem<ESZ>::type;
  const T* __restrict__ A = reinterpret_cast<const T*>(A_);
  T* __restrict__ out = reinterpret_cast<T*>(out_);
  __shared__ int32_t sidx[WS_IDX_CHUNK];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = r0 + rows_per_wg < m ? r0 + rows_per_wg : m;
  for (int c0 = 0; c0 < n_ws_pad; c0 += WS_IDX_CHUNK) {
    const int cn = n_ws_pad - c0 < WS_IDX_CHUNK ? n_ws_pad - c0 : WS_IDX_CHUNK;
    __syncthreads();                 // the readers of the previous chunk are done
    for (int c = tid; c < cn; c += WS_THREADS) {
      const int32_t j = c0 + c < n_ws ? idx[c0 + c] : -1;
      sidx[c] = (unsigned)j < (unsigned)n ? j : -1;                // padding and out-of-range entries: a zero column
    }
    __syncthreads();
    for (int64_t r = r0; r < r1; r += WS_ROWS) {
      for (int c = tid; c < cn; c += WS_THREADS) {
        const int32_t j = sidx[c];
        T v[WS_ROWS];
#pragma unroll
        for (int u = 0; u < WS_ROWS; ++u)
          v[u] = (j >= 0 && r + u < r1) ? __builtin_nontemporal_load(A + (r + u) * lda + j) : (T)0;
#pragma unroll
        for (int u = 0; u < WS_ROWS; ++u)
          if (r + u < r1) out[(r + u) * lda_ws + c0 + c] = v[u];
      }
    }
  }
}

// ---- KKT scan -----------------------------------------------------------------------------------------------------------------
// ONE workgroup of 16 waves walks the n coordinates in order, 1024 at a time: the excess and the violation flag per thread in the
// fp64 arithmetic the header states, a ballot per wave, the 16 wave counts through LDS, and every violator writes its index at
// (violators of earlier trips) + (of earlier waves) + (of lower lanes): increasing order, no atomics, the same bytes every run.
// n <= 16384 wherever the matrix-core pair is served: 16 trips over at most 1 MiB of gradients.
// Resources (gfx950, -O3): 41 VGPRs, 64 bytes of LDS, no scratch.
constexpr int KS_THREADS = 1024;
struct KktWeights { double a[BT_NV]; };

static __global__ __launch_bounds__(KS_THREADS) void kkt_scan_kernel(const float* __restrict__ G, int64_t n, int nv, KktWeights w,
                                                                     double one_plus_slack, const uint8_t* __restrict__ in_ws,
                                                                     const float* __restrict__ factor, float* __restrict__ excess,
                                                                     int32_t* __restrict__ viol_idx, int32_t* __restrict__ viol_count) {
  __shared__ int wcount[KS_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int running = 0;
  for (int64_t base = 0; base < n; base += KS_THREADS) {
    const int64_t i = base + tid;
    bool viol = false;
    double ex = 0.0;
    if (i < n && in_ws[i] == 0) {
      const double pf = factor ? (double)factor[i] : 1.0;
      for (int j = 0; j < nv; ++j) {
        const double a = (double)fabsf(G[(int64_t)j * n + i]);
        const double d = w.a[j] * pf;
        const double e = d > 0.0 ? a / d : (a > 0.0 ? (double)INFINITY : 0.0);
        ex = e > ex ? e : ex;
        viol = viol || a > d * one_plus_slack;
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

}  // namespace fos
