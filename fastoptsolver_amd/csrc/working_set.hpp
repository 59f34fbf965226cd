// Working-set solve of a sparse path (include/fos_working_set.h, include/fos_multinomial_ws.h): the column gather and the KKT
// scan of every loss family.  The lockstep runs on the gathered matrix as on any other fos_problem; these two kernels and the
// gradient entry points (existing launches) are all the outer loop of fastoptsolver_amd/working_set.py needs from the device.
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
// The 16 columns of a block are nv / C fits of C columns each ("segments": segment s is columns s*C .. s*C + C-1); C = 1 for
// every loss but the multinomial one, whose C class vectors are seen together (softmax_link.hpp has the same layout).
// ONE workgroup of 16 waves walks the n coordinates in order, 1024 at a time.  For coordinate i outside the set, per segment s,
// all in fp64 from the float G, p_i the bound penalty factor (or 1):
//     l1      v = max_c |G[s*C + c][i]|                                       violator: v > alpha1[s] p_i (1 + slack)
//     group   q = sum_c G[s*C + c][i]^2 (c ascending),  v = sqrt(q)           violator: q > (alpha1[s] p_i (1 + slack))^2
// (the grouped decision takes no square root: it is the comparison of the squares, exact in the products of the floats), and
// excess[i] = (float) max_s v / (alpha1[s] p_i); a zero denominator gives +inf where v > 0 and 0 where v = 0.  A ballot per wave,
// the 16 wave counts through LDS, and every violator writes its index at (violators of earlier trips) + (of earlier waves) +
// (of lower lanes): increasing order, no read-modify-write, the same bytes every run.  classes and grouped are the same for
// every lane.
// n <= 16384 wherever the matrix-core pair is served: 16 trips over at most 1 MiB of gradients.
// The body is written once.  ONE_COLUMN fixes C = 1, l1 at compile time (classes_ and grouped_ are not read): the two inner loops
// fold into one load per column, which the 16 loads of a coordinate need to be issued together (with C in a register the
// scan is a fifth slower: profiles/ws_refactor/README.md).  kkt_scan_kernel below is that instantiation;
// class_kkt_scan_kernel of multinomial_ws.hpp is the other.
constexpr int KS_THREADS = 1024;
struct ScanWeights { double a1[BT_NV]; };                            // per segment: what a scan kernel takes (128 bytes of kernarg)
struct ClassWeights : ScanWeights { double a2[BT_NV]; };             // what a call checks and the column pass of duality.hpp takes

template <bool ONE_COLUMN>
__device__ __forceinline__ void kkt_scan_body(const float* __restrict__ G, int64_t n, int nv, int classes_, int grouped_,
                                              const ScanWeights& w, double one_plus_slack, const uint8_t* __restrict__ in_ws,
                                              const float* __restrict__ factor, float* __restrict__ excess,
                                              int32_t* __restrict__ viol_idx, int32_t* __restrict__ viol_count) {
  __shared__ int wcount[KS_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int classes = ONE_COLUMN ? 1 : classes_;
  const bool grouped = ONE_COLUMN ? false : grouped_ != 0;
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
        if constexpr (ONE_COLUMN) {                      // the maximum over one entry is the entry (a NaN gives no violator and
          v = (double)fabsf(g[0]);                       // leaves the excess alone either way)
          viol = viol || v > thr;
        } else if (grouped) {
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

// The scan of fos_kkt_scan: every column a fit of its own, the l1 condition.
// Resources (gfx950, -O3): 43 VGPRs, 64 bytes of LDS, no scratch.
static __global__ __launch_bounds__(KS_THREADS) void kkt_scan_kernel(const float* __restrict__ G, int64_t n, int nv, ScanWeights w,
                                                                     double one_plus_slack, const uint8_t* __restrict__ in_ws,
                                                                     const float* __restrict__ factor, float* __restrict__ excess,
                                                                     int32_t* __restrict__ viol_idx, int32_t* __restrict__ viol_count) {
  kkt_scan_body<true>(G, n, nv, 1, 0, w, one_plus_slack, in_ws, factor, excess, viol_idx, viol_count);
}

}  // namespace fos
