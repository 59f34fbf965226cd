// The streaming gradient pass over a 28-bit copy of an fp32 A (12.5 % fewer HBM bytes than the raw rows).
//
// Format.  An element keeps bits 23:0 of its fp32 pattern (mantissa and the lowest exponent bit) and a nibble [sign | e3]
// with (biased exponent) >> 1 == E0/2 + e3: a window of 16 binades that starts at the even exponent E0, chosen per matrix.
// A packed row is laid out for ONE geometry of THREADS threads, thread t owning columns 16t .. 16t+15: three planes of
// THREADS x 16 bytes and one of THREADS x 8 bytes (56 bytes per thread instead of 64), so every load instruction of a wave
// is one contiguous run.  Group g (columns 4g .. 4g+3 of the thread, elements a b c d) is dword g of each 16-byte plane:
//   plane0[g] = a[23:0] | d[7:0] << 24,   plane1[g] = b[23:0] | d[15:8] << 24,   plane2[g] = c[23:0] | d[23:16] << 24
// and byte k of dword h of the nibble plane holds element k of group 2h (low nibble) and of group 2h+1 (high nibble).
// Decode: 4 VALU instructions turn four nibbles into the four top bytes [sign | exponent >> 1], then one v_perm_b32 each for
// a, b, c and three for d - 10 per 4 elements, all exact.  Threads beyond n read zero bytes against a zero slice of y.
//
// The pass.  Drained, in bursts of R rows from one register tile: R x 56 bytes per thread in flight, then one barrier and one
// cross-wave ladder for the R rows (see gemv_packed_kernel).  R is the planner's (fos_plan.hip pack_rows: what measured
// fastest per geometry and row order) or FOS_PLAN_PACK_ROWS; the result does not depend on it bit for bit.
//
// Exceptions.  An element outside the window (zero, denormal, too small, too large) is stored as an in-window placeholder and
// listed in a sparse D with A = P + D exactly (two entries per exception, +true and -placeholder, so nothing is rounded at
// pack time).  D never enters the streaming loop: pk_bprime_kernel forms b' = b - D y before the pass, the pass runs on b'
// (its residual r = P y - b' is then the true residual) and stores r, pk_dtr_kernel adds D^T r to the first slab afterwards.
// Both sparse kernels sum in fp64 in a fixed order: the result is deterministic, and differs from the raw pass only by the
// association of the ~1e-4 of the products that are exceptions.
#pragma once
#include "gemv_pair.hpp"

namespace fos {
namespace pk {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int CPT = 16;                      // columns per thread
constexpr int BYTES_PER_THREAD = 56;         // of one packed row
constexpr unsigned E0_MAX = 238;             // even; E0 + 15 stays a finite exponent

__host__ __device__ inline int64_t row_bytes(int threads) { return (int64_t)threads * BYTES_PER_THREAD; }

// ---- pack arithmetic (host and device; tests/test_packed_format.py mirrors it in NumPy) ---------------------------------
__host__ __device__ inline bool in_window(unsigned bits, unsigned e0) {
  const unsigned ex = (bits >> 23) & 0xffu;
  return ex >= e0 && ex <= e0 + 15u;
}
// the stored stand-in of an out-of-window element: same sign and mantissa, exponent clamped to the window's nearer end
__host__ __device__ inline unsigned placeholder(unsigned bits, unsigned e0) {
  const unsigned ex = (bits >> 23) & 0xffu;
  return (bits & 0x807fffffu) | ((ex < e0 ? e0 : e0 + 15u) << 23);
}
__host__ __device__ inline unsigned nibble_of(unsigned bits, unsigned e0) {       // bits in the window
  return ((bits >> 31) << 3) | ((((bits >> 23) & 0xffu) - e0) >> 1);
}
// 16 in-window bit patterns of one thread -> its 12 plane dwords (pl[plane][group]) and 2 nibble dwords
__host__ __device__ inline void pack16(const unsigned (&bits)[CPT], unsigned e0, unsigned (&pl)[3][4], unsigned (&nb)[2]) {
  nb[0] = nb[1] = 0;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const unsigned d = bits[4 * g + 3];
    pl[0][g] = (bits[4 * g] & 0xffffffu) | ((d & 0xffu) << 24);
    pl[1][g] = (bits[4 * g + 1] & 0xffffffu) | (((d >> 8) & 0xffu) << 24);
    pl[2][g] = (bits[4 * g + 2] & 0xffffffu) | (((d >> 16) & 0xffu) << 24);
#pragma unroll
    for (int k = 0; k < 4; ++k) nb[g >> 1] |= nibble_of(bits[4 * g + k], e0) << (8u * k + 4u * (g & 1));
  }
}

// ---- decode -------------------------------------------------------------------------------------------------------------
// top bytes [sign | exponent >> 1] of four elements from their nibbles (one per byte; the byte's upper nibble is ignored)
__device__ inline unsigned top_bytes(unsigned w, unsigned e0h4) {
  unsigned t = w & 0x0F0F0F0Fu;
  t += 0x78787878u;                          // the sign (nibble bit 3) carries into bit 7; a clear one leaves 1111 in bits 6:3
  t &= 0x87878787u;
  return t + e0h4;                           // E0/2 + 7 < 128: no carry into the sign
}
__device__ inline void decode_group(unsigned p0, unsigned p1, unsigned p2, unsigned top, float (&f)[4]) {
  f[0] = __uint_as_float(__builtin_amdgcn_perm(top, p0, 0x04020100u));
  f[1] = __uint_as_float(__builtin_amdgcn_perm(top, p1, 0x05020100u));
  f[2] = __uint_as_float(__builtin_amdgcn_perm(top, p2, 0x06020100u));
  const unsigned d01 = __builtin_amdgcn_perm(p1, p0, 0x0c0c0703u);
  const unsigned d012 = __builtin_amdgcn_perm(p2, d01, 0x0c070100u);
  f[3] = __uint_as_float(__builtin_amdgcn_perm(top, d012, 0x07020100u));
}
__device__ inline u32x2 load8nt(const void* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p)); }

// ---- the pass -----------------------------------------------------------------------------------------------------------
// slab[w] = sum over the rows of workgroup w of P_i^T (P_i . y - b_i),  r_out[i] = P_i . y - b_i,  rr_part[w] = sum r_i^2.
// Rows: contiguous blocks of rows_per_wg (IL = false) or dealt round-robin (IL = true); step s of workgroup w is row
// row_lo + first + s * group.  The loop is DRAINED and works in bursts of R steps from ONE register tile:
//   issue the loads of R rows (rows past the end clamped, not predicated: loaded and weighted by zero); s_waitcnt vmcnt(0);
//   per row: decode, the dot with y (v_pk_fma_f32, acc0 / acc1), the wave sum, lane 0 -> red[pb][r][wave];
//   ONE barrier; lanes 16r .. 16r+NW-1 read row r's partials (all others 0); ONE row_shr 1/2/4/8 ladder leaves the sum of
//   row r in lane 16r+15, a readlane per row; then per row, in step order: s -= b, rr += s^2, r_out, gv += a[r] * s
// with the decoded a[R][8] kept in registers across the barrier, so nothing is decoded twice.  The load latency, the barrier,
// the LDS round trip and the cross-wave ladder are paid once per R * 56 * THREADS bytes in flight instead of once per row:
// that, not overlap (a wave never computes while its own loads are in flight), is what R buys - profiles/packed/README.md.
// Every row sees the same operations in the same order for every R (the 16-lane ladder is the 64-lane wave_sum of one
// partial per lane without its additions of zero), so slabs, rr_part and r_out do not depend on R bit for bit.
// ADJ (IL only; the probe's variant, no product launch uses it) takes the rows of a burst adjacent in memory instead:
// workgroup w owns rows R*(w + k*grid) .. +R-1.  That changes which rows a workgroup sums, so its bits depend on R.
// Requirements (checked on the host): n % 16 == 0, n <= 16 * THREADS, P 16-byte aligned with rows of row_bytes(THREADS).
constexpr int MAX_ROWS = 4;                  // rows per burst: one 16-lane DPP row each

template <int THREADS, bool IL, int R, bool ADJ = false>
__global__ __launch_bounds__(THREADS, THREADS / 256) void gemv_packed_kernel(
    const unsigned char* __restrict__ P, const float* __restrict__ b, int64_t m, int n, YSource ys, unsigned e0h4,
    int64_t rows_per_wg, float* __restrict__ slabs, float* __restrict__ r_out, double* __restrict__ rr_part) {
  constexpr int NW = THREADS / 64;
  static_assert(NW >= 8 && NW <= 16 && R >= 1 && R <= MAX_ROWS, "the partials of one row fill at most one 16-lane DPP row");
  static_assert(IL || !ADJ, "rows of a block are adjacent already");
  __shared__ float red[2][R][NW];

  if (ys.stopped != nullptr && *ys.stopped != 0) return;
  if (ys.t_stamp != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *ys.t_stamp = wall_clock64();

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row_lo = IL ? 0 : (int64_t)blockIdx.x * rows_per_wg;
  int64_t row_hi = IL ? m : row_lo + rows_per_wg;
  if (row_hi > m) row_hi = m;

  const int col = tid * CPT;
  const bool live = col < n;                 // n % 16 == 0: a thread is wholly live or wholly dead
  f32x2 yv[CPT / 2], gv[CPT / 2];
#pragma unroll
  for (int e = 0; e < CPT / 2; ++e) { yv[e] = f32x2{0.f, 0.f}; gv[e] = f32x2{0.f, 0.f}; }
  if (live) {
    const double beta = source_beta(ys);
#pragma unroll
    for (int q = 0; q < CPT / 4; ++q) {
      if (ys.y != nullptr) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(ys.y + col + 4 * q);
        yv[2 * q] = f32x2{t.x, t.y}; yv[2 * q + 1] = f32x2{t.z, t.w};
      } else {                               // the same form_y as the update kernel: both kernels see the same y_k
        yv[2 * q] = f32x2{(float)source_y(ys, col + 4 * q, beta), (float)source_y(ys, col + 4 * q + 1, beta)};
        yv[2 * q + 1] = f32x2{(float)source_y(ys, col + 4 * q + 2, beta), (float)source_y(ys, col + 4 * q + 3, beta)};
      }
    }
  }

  const int64_t nrows = row_hi - row_lo;     // may be <= 0 for trailing workgroups
  const int64_t group = IL ? gridDim.x : 1;
  const int64_t first = IL ? (int64_t)blockIdx.x : 0;
  const int64_t nsteps = nrows > first ? (nrows - first + group - 1) / group : 0;
  const int64_t nbursts = ADJ ? (nrows > first * R ? (nrows - first * R + group * R - 1) / (group * R) : 0) : (nsteps + R - 1) / R;
  auto row_of = [&](int64_t k, int r) -> int64_t {       // row of step k*R + r; at or past row_hi beyond the last step
    return ADJ ? (first + k * group) * R + r : row_lo + first + (k * R + r) * group;
  };
  const int64_t rbytes = row_bytes(THREADS);
  const unsigned voff16 = (unsigned)tid * 16u, voff8 = (unsigned)THREADS * 48u + (unsigned)tid * 8u;
  double rr = 0.0;

  u32x4 tile[R][3];
  u32x2 nib[R];
  float bval[R];
  const float* b_src = b != nullptr ? b : reinterpret_cast<const float*>(P);   // dummy source, discarded by select
  for (int64_t k = 0; k < nbursts; ++k) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      int64_t row = row_of(k, r);
      if (row >= row_hi) row = row_hi - 1;   // clamp: loaded but weighted by zero below (nbursts > 0: the workgroup has a row)
      bval[r] = b_src[b != nullptr ? row : 0];
      const unsigned char* rp = P + row * rbytes;
#pragma unroll
      for (int c = 0; c < 3; ++c) tile[r][c] = load16<true>(rp + voff16 + (unsigned)c * THREADS * 16u);
      nib[r] = load8nt(rp + voff8);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    f32x2 a[R][CPT / 2];
    const int pb = (int)(k & 1);
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const unsigned w = (g >> 1) ? nib[r].y : nib[r].x;
        const unsigned top = top_bytes((g & 1) ? (w >> 4) : w, e0h4);
        float f[4];
        decode_group(tile[r][0][g], tile[r][1][g], tile[r][2][g], top, f);
        a[r][2 * g] = f32x2{f[0], f[1]}; a[r][2 * g + 1] = f32x2{f[2], f[3]};
      }
      f32x2 acc0 = f32x2{0.f, 0.f}, acc1 = f32x2{0.f, 0.f};
#pragma unroll
      for (int e = 0; e < CPT / 2; e += 2) {
        acc0 = __builtin_elementwise_fma(a[r][e], yv[e], acc0);
        acc1 = __builtin_elementwise_fma(a[r][e + 1], yv[e + 1], acc1);
      }
      acc0 += acc1;
      const float part = wave_sum(acc0.x + acc0.y);
      if (lane == 0) red[pb][r][wave] = part;
    }
    __syncthreads();                         // red[pb] is written again two bursts on, behind the next burst's barrier
    float v = ((lane >> 4) < R && (lane & 15) < NW) ? red[pb][lane >> 4][lane & 15] : 0.f;
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, false));   // row_shr:1
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xF, 0xF, false));   // row_shr:2
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xF, 0xF, false));   // row_shr:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xF, 0xF, false));   // row_shr:8
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float s = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16 * r + 15));
      const int64_t row = row_of(k, r);
      const float bi = b != nullptr ? bval[r] : 0.f;
      if (row < row_hi) {
        s -= bi;
        rr += (double)s * (double)s;
        if (tid == 0) r_out[row] = s;
      } else {
        s = 0.f;
      }
      const f32x2 s2 = f32x2{s, s};
#pragma unroll
      for (int e = 0; e < CPT / 2; ++e) gv[e] = __builtin_elementwise_fma(a[r][e], s2, gv[e]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }

  if (live) {
    float* slab = slabs + (int64_t)blockIdx.x * n + col;
#pragma unroll
    for (int q = 0; q < CPT / 4; ++q)
      *reinterpret_cast<f32x4*>(slab + 4 * q) = f32x4{gv[2 * q].x, gv[2 * q].y, gv[2 * q + 1].x, gv[2 * q + 1].y};
  }
  if (tid == 0) rr_part[blockIdx.x] = rr;
}

// ---- the packer ---------------------------------------------------------------------------------------------------------
// One thread per (row, 16-column group).  COUNT: row_cnt[row] += exceptions of the group, flags[0] |= 1 on an inf / NaN;
// nothing is written to P.  Otherwise: the packed row (dead groups: zero bytes), and every exception at a free slot of its
// row's CSR segment (row_cnt then counts the slots handed out; the order within a row is put right on the host).
template <bool COUNT>
__global__ __launch_bounds__(256) void pack_rows_kernel(const float* __restrict__ A, int64_t lda, int64_t m, int n, int threads,
                                                        unsigned e0, unsigned char* __restrict__ P, int* __restrict__ row_cnt,
                                                        unsigned* __restrict__ flags, const int* __restrict__ csr_ptr,
                                                        int* __restrict__ csr_col, float* __restrict__ csr_tv,
                                                        float* __restrict__ csr_pv) {
  const int64_t total = m * threads;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / threads;
    const int t = (int)(i % threads);
    unsigned pl[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    unsigned nb[2] = {0, 0};
    if (t * CPT < n) {
      const float* ap = A + row * lda + (int64_t)t * CPT;
      unsigned bits[CPT];
#pragma unroll
      for (int q = 0; q < CPT / 4; ++q) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(ap + 4 * q);
        bits[4 * q] = v.x; bits[4 * q + 1] = v.y; bits[4 * q + 2] = v.z; bits[4 * q + 3] = v.w;
      }
      int nex = 0;
      bool bad = false;
#pragma unroll
      for (int e = 0; e < CPT; ++e) {
        if (in_window(bits[e], e0)) continue;
        ++nex;
        bad |= ((bits[e] >> 23) & 0xffu) == 0xffu;
        if constexpr (!COUNT) {
          const unsigned ph = placeholder(bits[e], e0);
          const int slot = csr_ptr[row] + atomicAdd(&row_cnt[row], 1);
          csr_col[slot] = t * CPT + e;
          csr_tv[slot] = __uint_as_float(bits[e]);
          csr_pv[slot] = __uint_as_float(ph);
          bits[e] = ph;
        }
      }
      if constexpr (COUNT) {
        if (nex) atomicAdd(&row_cnt[row], nex);
        if (bad) atomicOr(flags, 1u);
      } else {
        pack16(bits, e0, pl, nb);
      }
    }
    if constexpr (!COUNT) {
      unsigned char* rp = P + row * row_bytes(threads);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        *reinterpret_cast<u32x4*>(rp + (int64_t)c * threads * 16 + (int64_t)t * 16) = u32x4{pl[c][0], pl[c][1], pl[c][2], pl[c][3]};
      *reinterpret_cast<u32x2*>(rp + (int64_t)threads * 48 + (int64_t)t * 8) = u32x2{nb[0], nb[1]};
    }
  }
}

// ---- the two sparse launches around the pass ------------------------------------------------------------------------------
// b'_i = b_i - sum_j D_ij y_j  (thread per row; y as the pass forms it: fp64 form_y rounded once to fp32; fp64 sum)
static __global__ __launch_bounds__(256) void pk_bprime_kernel(const int* __restrict__ csr_ptr, const int* __restrict__ csr_col,
                                                              const float* __restrict__ csr_tv, const float* __restrict__ csr_pv,
                                                              const float* __restrict__ b, int64_t m, YSource ys,
                                                              float* __restrict__ bprime) {
  if (ys.stopped != nullptr && *ys.stopped != 0) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const double beta = source_beta(ys);
  double acc = 0.0;
  for (int k = csr_ptr[i]; k < csr_ptr[i + 1]; ++k) {
    const double y = (double)(float)source_y(ys, csr_col[k], beta);
    acc = fma((double)csr_tv[k], y, acc);
    acc = fma(-(double)csr_pv[k], y, acc);
  }
  bprime[i] = (float)((b != nullptr ? (double)b[i] : 0.0) - acc);
}
// slab0[j] += sum_i D_ij r_i  (one WAVE per column: lane l takes entries l, l + 64, ... of the column, rows ascending, then the
// DPP ladder - a fixed order; columns without an exception are not touched.  A thread per column walked ~100 dependent-latency
// gathers of r at 64 GiB.)
static __global__ __launch_bounds__(256) void pk_dtr_kernel(const int* __restrict__ csc_ptr, const int* __restrict__ csc_row,
                                                           const float* __restrict__ csc_tv, const float* __restrict__ csc_pv,
                                                           const float* __restrict__ r, int n, const int* stopped,
                                                           float* __restrict__ slab0) {
  if (stopped != nullptr && *stopped != 0) return;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= n) return;                        // wave-uniform, like the next one
  const int lo = csc_ptr[j], hi = csc_ptr[j + 1];
  if (lo == hi) return;
  double acc = 0.0;
  for (int k = lo + lane; k < hi; k += 64) {
    const double ri = (double)r[csc_row[k]];
    acc = fma((double)csc_tv[k], ri, acc);
    acc = fma(-(double)csc_pv[k], ri, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) slab0[j] = (float)((double)slab0[j] + acc);
}

}  // namespace pk
}  // namespace fos
