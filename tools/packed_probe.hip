// Step-1 probe for a 28-bit packed copy of fp32 A (not part of the product library).
//   hipcc -O3 --offload-arch=gfx950 -o tools/packed_probe tools/packed_probe.hip && ./tools/packed_probe [m] [iters] [rounds] [n]
// Row width n = 16384 (the 1024-thread geometry of the headline) or 8192 (512 threads).  In ONE process, interleaved rounds:
//   loads_raw   : loads-only pass over the raw fp32 buffer
//   loads_pack  : loads-only pass over the packed buffer (0.875 x the bytes)
//   raw_body    : the library's instantiation of fos::gemv_pair_kernel for that width, rows ordered as the planner would
//   packed_body : loads + decode + both products from the packed copy, no exceptions (out-of-window elements are
//                 clamped into the window in BOTH buffers before anything is timed, so both bodies see the same matrix):
//                 one row per drain from two register tiles, the library's pass before it worked in bursts
//   rowsR       : the library's fos::pk::gemv_packed_kernel with R rows per burst (1, 2, 3 at 1024 threads; 2, 3, 4 at 512)
//   rowsR_adj   : the same with the rows of a burst adjacent in memory (interleaved row order only; not bit-identical)
// All bodies are checked against the two-pass fp64-accumulating fallback kernels, and every rowsR bit for bit against packed_body.
// Last lines: each variant against packed_body and the stop rule (median faster by 5 x packed_body's max - min).
//
// Packed format (one row = 3 planes of THREADS*16 bytes + 1 plane of THREADS*8 bytes; thread t owns columns 16t..16t+15):
//   see fastoptsolver_amd/csrc/gemv_packed.hpp, whose kernel and packer this probe runs.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>
#include "../fastoptsolver_amd/csrc/gemv_packed.hpp"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

namespace pk = fos::pk;

// Clamp every out-of-window exponent of A into [E0, E0+15] IN PLACE (the probe times no exceptions); counts[0] += clamped.
__global__ __launch_bounds__(256) void clamp_window(float* __restrict__ A, size_t count, unsigned e0, unsigned long long* counts) {
  unsigned long long clamped = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned u = __float_as_uint(A[i]);
    if (!pk::in_window(u, e0)) { A[i] = __uint_as_float(pk::placeholder(u, e0)); ++clamped; }
  }
  if (clamped) atomicAdd(counts, clamped);
}

__global__ void fill_normal(float* p, size_t n, unsigned seed) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    unsigned long long z = (i + 1) * 0x9E3779B97F4A7C15ull + seed * 0xD1B54A32D192ED03ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31;
    float u1 = ((unsigned)(z & 0xffffffffu) + 1.0f) * 2.3283064e-10f;
    float u2 = (unsigned)(z >> 32) * 2.3283064e-10f;
    p[i] = sqrtf(-2.0f * logf(u1)) * cosf(6.2831853f * u2);
  }
}

// loads only, 16 bytes per lane, grid-stride (nvec 16-byte vectors)
__global__ __launch_bounds__(256) void stream_sum(const fos::u32x4* __restrict__ p, size_t nvec, float* out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (; i + 3 * stride < nvec; i += 4 * stride) {
    fos::u32x4 a = fos::load16<true>(p + i), b = fos::load16<true>(p + i + stride), c = fos::load16<true>(p + i + 2 * stride),
               d = fos::load16<true>(p + i + 3 * stride);
    acc += __uint_as_float(a.x ^ b.y ^ c.z ^ d.w);
  }
  for (; i < nvec; i += stride) acc += __uint_as_float(fos::load16<true>(p + i).x);
  if (acc == 123.456f) out[0] = acc;
}

__global__ void reduce_slabs(const float* slabs, int nslabs, int n, float* g) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double acc = 0.0;
  for (int s = 0; s < nslabs; ++s) acc += (double)slabs[(size_t)s * n + j];
  g[j] = (float)acc;
}

// packed_body, the baseline of the rows-per-burst stop rule: the pass as the library had it before it worked in bursts, kept here
// so that the tables in profiles/packed/README.md can be taken again.  One row per drain, TWO register tiles (the second buys
// nothing in a drained loop), a 64-lane ladder for the cross-wave sum.
namespace fos {
namespace pk {
template <int THREADS, bool IL>
__global__ __launch_bounds__(THREADS, THREADS / 256) void packed_2tile_kernel(
    const unsigned char* __restrict__ P, const float* __restrict__ b, int64_t m, int n, YSource ys, unsigned e0h4,
    int64_t rows_per_wg, float* __restrict__ slabs, float* __restrict__ r_out, double* __restrict__ rr_part) {
  constexpr int NW = THREADS / 64;
  constexpr int NBUF = 2;
  static_assert(NW >= 8 && NW <= 64, "one partial per lane in the cross-wave sum");
  __shared__ float red[2][NW];

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
  const int64_t rbytes = row_bytes(THREADS);
  const unsigned voff16 = (unsigned)tid * 16u, voff8 = (unsigned)THREADS * 48u + (unsigned)tid * 8u;
  double rr = 0.0;

  u32x4 tile[NBUF][3];
  u32x2 nib[NBUF];
  float bval[NBUF];
  const float* b_src = b != nullptr ? b : reinterpret_cast<const float*>(P);   // dummy source, discarded by select
  auto issue = [&](int buf, int64_t step) {
    int64_t row = row_lo + first + step * group;
    if (row >= row_hi) row = row_hi - 1;     // clamp: loaded but weighted by zero below
    bval[buf] = b_src[b != nullptr ? row : 0];
    const unsigned char* rp = P + row * rbytes;
#pragma unroll
    for (int c = 0; c < 3; ++c) tile[buf][c] = load16<true>(rp + voff16 + (unsigned)c * THREADS * 16u);
    nib[buf] = load8nt(rp + voff8);
  };
  auto consume = [&](int buf, int64_t step) {
    f32x2 a[CPT / 2];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const unsigned w = (g >> 1) ? nib[buf].y : nib[buf].x;
      const unsigned top = top_bytes((g & 1) ? (w >> 4) : w, e0h4);
      float f[4];
      decode_group(tile[buf][0][g], tile[buf][1][g], tile[buf][2][g], top, f);
      a[2 * g] = f32x2{f[0], f[1]}; a[2 * g + 1] = f32x2{f[2], f[3]};
    }
    f32x2 acc0 = f32x2{0.f, 0.f}, acc1 = f32x2{0.f, 0.f};
#pragma unroll
    for (int e = 0; e < CPT / 2; e += 2) {
      acc0 = __builtin_elementwise_fma(a[e], yv[e], acc0);
      acc1 = __builtin_elementwise_fma(a[e + 1], yv[e + 1], acc1);
    }
    acc0 += acc1;
    const float part = wave_sum(acc0.x + acc0.y);
    const int pb = (int)(step & 1);
    if (lane == 0) red[pb][wave] = part;
    __syncthreads();
    float s = wave_sum(lane < NW ? red[pb][lane] : 0.f);
    const int64_t row = row_lo + first + step * group;
    const float bi = b != nullptr ? bval[buf] : 0.f;
    if (row < row_hi) {
      s -= bi;
      rr += (double)s * (double)s;
      if (tid == 0) r_out[row] = s;
    } else {
      s = 0.f;
    }
    const f32x2 s2 = f32x2{s, s};
#pragma unroll
    for (int e = 0; e < CPT / 2; ++e) gv[e] = __builtin_elementwise_fma(a[e], s2, gv[e]);
  };

  if (nsteps > 0) {
    issue(0, 0);
    int64_t s = 0;
    for (; s + NBUF <= nsteps; s += NBUF) {
#pragma unroll
      for (int u = 0; u < NBUF; ++u) {
        issue((u + NBUF - 1) % NBUF, s + u + NBUF - 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        consume(u, s + u);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (s < nsteps) consume(0, s);           // its tile is already in flight
  }

  if (live) {
    float* slab = slabs + (int64_t)blockIdx.x * n + col;
#pragma unroll
    for (int q = 0; q < CPT / 4; ++q)
      *reinterpret_cast<f32x4*>(slab + 4 * q) = f32x4{gv[2 * q].x, gv[2 * q].y, gv[2 * q + 1].x, gv[2 * q + 1].y};
  }
  if (tid == 0) rr_part[blockIdx.x] = rr;
}
}  // namespace pk
}  // namespace fos

// the library's streaming instantiation for full rows of 16 * THREADS columns (fos_plan.hip kMenu): 1024 x 4 chunks, two
// tiles, drained; 512 x 4 chunks, three tiles
template <int THREADS, bool IL>
void launch_raw(const float* A, const float* b, int64_t m, int n, fos::YSource ys, int64_t rpw, float* slabs, double* rr, int nwg,
                hipStream_t st) {
  if constexpr (THREADS == 1024)
    hipLaunchKernelGGL((fos::gemv_pair_kernel<float, 1024, 4, 1, true, 4, true, 2, IL, false, true>), dim3(nwg), dim3(1024), 0, st, A,
                       (int64_t)n, b, m, n, ys, rpw, slabs, rr, (double*)nullptr);
  else
    hipLaunchKernelGGL((fos::gemv_pair_kernel<float, 512, 4, 1, true, 2, true, 3, IL, false, false>), dim3(nwg), dim3(512), 0, st, A,
                       (int64_t)n, b, m, n, ys, rpw, slabs, rr, (double*)nullptr);
}

template <int THREADS>
int run(int64_t m, int iters, int rounds) {
  const int n = THREADS * pk::CPT;
  const unsigned e0 = 114;                   // biased exponents 114..129: |a| in [2^-13, 8)
  const bool il = (size_t)m * n * 4 >= ((size_t)12 << 30);      // the planner's row order for this size (il_default)
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int nwg = prop.multiProcessorCount;
  const size_t raw_bytes = (size_t)m * n * 4, pk_bytes = (size_t)m * THREADS * pk::BYTES_PER_THREAD;
  printf("device %s  CUs %d  m %lld n %d  rows %s  raw %.2f GiB  packed %.2f GiB\n", prop.name, nwg, (long long)m, n, il ? "interleaved" : "blocks",
         (double)raw_bytes / (1 << 30), (double)pk_bytes / (1 << 30));
  float *A, *b, *y, *slabs, *g, *gref, *rout;
  unsigned char* P;
  double *rvec, *rr;
  unsigned long long* counts;
  CK(hipMalloc(&A, raw_bytes));
  CK(hipMalloc(&P, pk_bytes));
  CK(hipMalloc(&b, (size_t)m * 4));
  CK(hipMalloc(&rout, (size_t)m * 4));
  CK(hipMalloc(&y, (size_t)n * 4));
  CK(hipMalloc(&rvec, (size_t)m * 8));
  CK(hipMalloc(&slabs, (size_t)nwg * n * 4));
  CK(hipMalloc(&g, (size_t)n * 4));
  CK(hipMalloc(&gref, (size_t)n * 4));
  CK(hipMalloc(&rr, 2048 * sizeof(double)));
  CK(hipMalloc(&counts, 8));
  CK(hipMemset(counts, 0, 8));
  fill_normal<<<4096, 256>>>(A, (size_t)m * n, 1);
  fill_normal<<<256, 256>>>(b, (size_t)m, 2);
  fill_normal<<<32, 256>>>(y, (size_t)n, 3);
  int* row_cnt;
  CK(hipMalloc(&row_cnt, (size_t)m * 4));
  clamp_window<<<4096, 256>>>(A, (size_t)m * n, e0, counts);
  pk::pack_rows_kernel<false><<<4096, 256>>>(A, (int64_t)n, m, n, THREADS, e0, P, row_cnt, nullptr, nullptr, nullptr, nullptr, nullptr);
  CK(hipDeviceSynchronize());
  unsigned long long hcount = 0;
  CK(hipMemcpy(&hcount, counts, 8, hipMemcpyDeviceToHost));
  printf("out-of-window elements clamped: %llu of %.3e (%.3e)\n", hcount, (double)m * n, (double)hcount / ((double)m * n));

  hipStream_t st;
  CK(hipStreamCreate(&st));
  hipEvent_t e0v, e1v;
  CK(hipEventCreate(&e0v));
  CK(hipEventCreate(&e1v));
  fos::YSource ys{y, nullptr, nullptr, nullptr, nullptr, 0.0, nullptr};
  const unsigned e0h4 = (e0 >> 1) * 0x01010101u;
  const int64_t rpw = (m + nwg - 1) / nwg;

  auto run_raw = [&] {
    if (il) launch_raw<THREADS, true>(A, b, m, n, ys, rpw, slabs, rr, nwg, st);
    else launch_raw<THREADS, false>(A, b, m, n, ys, rpw, slabs, rr, nwg, st);
  };
  auto run_packed = [&] {
    auto kern = il ? pk::packed_2tile_kernel<THREADS, true> : pk::packed_2tile_kernel<THREADS, false>;
    hipLaunchKernelGGL(kern, dim3(nwg), dim3(THREADS), 0, st, (const unsigned char*)P, (const float*)b, m, n, ys, e0h4, rpw, slabs,
                       rout, rr);
  };
  auto run_loads_raw = [&] { stream_sum<<<nwg * 8, 256, 0, st>>>((const fos::u32x4*)A, raw_bytes / 16, g); };
  auto run_loads_pack = [&] { stream_sum<<<nwg * 8, 256, 0, st>>>((const fos::u32x4*)P, pk_bytes / 16, g); };

  // reference gradient on the clamped matrix: the two-pass fallback (fp64 accumulation)
  std::vector<float> href(n), hg(n);
  {
    const int chunks = 64;
    const int64_t rpc = (m + chunks - 1) / chunks;
    float* slabs_ref;
    CK(hipMalloc(&slabs_ref, (size_t)chunks * n * 4));
    hipLaunchKernelGGL(fos::residual_rows_kernel<float>, dim3(2048), dim3(256), 0, st, A, (int64_t)n, b, m, n, ys, rvec, rr);
    hipLaunchKernelGGL(fos::transpose_rows_kernel<float>, dim3((n + 255) / 256, chunks), dim3(256), 0, st, A, (int64_t)n, m, n,
                       rvec, (const int*)nullptr, rpc, slabs_ref);
    reduce_slabs<<<(n + 255) / 256, 256, 0, st>>>(slabs_ref, chunks, n, gref);
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(href.data(), gref, (size_t)n * 4, hipMemcpyDeviceToHost));
    CK(hipFree(slabs_ref));
  }
  double refnorm = 0;
  for (float v : href) refnorm += (double)v * v;
  refnorm = std::sqrt(refnorm);
  auto check = [&](const char* name) {
    reduce_slabs<<<(n + 255) / 256, 256, 0, st>>>(slabs, nwg, n, g);
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(hg.data(), g, (size_t)n * 4, hipMemcpyDeviceToHost));
    double err = 0;
    for (int j = 0; j < n; ++j) err += ((double)hg[j] - href[j]) * ((double)hg[j] - href[j]);
    printf("%-12s gradient relerr vs fp64 two-pass %.3e\n", name, std::sqrt(err) / refnorm);
  };
  run_raw();
  check("raw_body");
  run_packed();
  check("packed_body");
  {   // the stored residuals of the packed pass against the fp64 ones
    std::vector<float> hr(m);
    std::vector<double> hrd(m);
    CK(hipMemcpy(hr.data(), rout, (size_t)m * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hrd.data(), rvec, (size_t)m * 8, hipMemcpyDeviceToHost));
    double e = 0, nn = 0;
    for (int64_t i = 0; i < m; ++i) { e += (hr[i] - hrd[i]) * (hr[i] - hrd[i]); nn += hrd[i] * hrd[i]; }
    printf("packed_body  residual relerr vs fp64 %.3e\n", std::sqrt(e / nn));
  }

  // the library's pass with R rows per burst: R = 1, 2, 3 at 1024 threads, 2, 3, 4 at 512; strided (the library's row assignment) and, where the rows
  // are interleaved, adjacent.  Each strided variant must reproduce packed_body bit for bit (slabs, stored r, rr partials).
  constexpr int RA = THREADS == 1024 ? 1 : 2;
  auto launch_rows = [&](int R, bool adj) {
    auto go = [&](auto kern) {
      hipLaunchKernelGGL(kern, dim3(nwg), dim3(THREADS), 0, st, (const unsigned char*)P, (const float*)b, m, n, ys, e0h4, rpw, slabs,
                         rout, rr);
    };
    auto pick = [&](auto rc) {
      constexpr int RR = decltype(rc)::value;
      if (!il) go(pk::gemv_packed_kernel<THREADS, false, RR>);
      else if (adj) go(pk::gemv_packed_kernel<THREADS, true, RR, true>);
      else go(pk::gemv_packed_kernel<THREADS, true, RR>);
    };
    if (R == RA) pick(std::integral_constant<int, RA>{});
    else if (R == RA + 1) pick(std::integral_constant<int, RA + 1>{});
    else pick(std::integral_constant<int, RA + 2>{});
  };
  {
    std::vector<float> s0((size_t)nwg * n), s1((size_t)nwg * n), r0(m), r1(m);
    std::vector<double> q0(nwg), q1(nwg);
    run_packed();
    CK(hipStreamSynchronize(st));
    CK(hipMemcpy(s0.data(), slabs, s0.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(r0.data(), rout, (size_t)m * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(q0.data(), rr, (size_t)nwg * 8, hipMemcpyDeviceToHost));
    for (int R = RA; R < RA + 3; ++R)
      for (int adj = 0; adj <= (il ? 1 : 0); ++adj) {
        CK(hipMemsetAsync(slabs, 0xff, s0.size() * 4, st));
        CK(hipMemsetAsync(rout, 0xff, (size_t)m * 4, st));
        launch_rows(R, adj != 0);
        char name[32];
        snprintf(name, sizeof name, "rows%d%s", R, adj ? "_adj" : "");
        check(name);
        CK(hipMemcpy(s1.data(), slabs, s1.size() * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(r1.data(), rout, (size_t)m * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(q1.data(), rr, (size_t)nwg * 8, hipMemcpyDeviceToHost));
        const bool same = !memcmp(s0.data(), s1.data(), s0.size() * 4) && !memcmp(r0.data(), r1.data(), (size_t)m * 4) &&
                          !memcmp(q0.data(), q1.data(), (size_t)nwg * 8);
        const bool same_r = !memcmp(r0.data(), r1.data(), (size_t)m * 4);
        printf("%-12s bitwise vs packed_body: slabs+r+rr %s, stored r %s\n", name, same ? "IDENTICAL" : "differ", same_r ? "IDENTICAL" : "differ");
        if (!adj && !same) { fprintf(stderr, "the strided burst is not bit-identical with packed_body\n"); return 1; }
      }
  }

  struct Var { std::string name; double bytes; int R; bool adj; std::vector<double> us; };
  std::vector<Var> vars = {{"loads_raw", (double)raw_bytes, 0, false, {}}, {"loads_pack", (double)pk_bytes, 0, false, {}},
                           {"raw_body", (double)raw_bytes, 0, false, {}}, {"packed_body", (double)pk_bytes, 0, false, {}}};
  for (int adj = 0; adj <= (il ? 1 : 0); ++adj)
    for (int R = RA; R < RA + 3; ++R)
      vars.push_back({"rows" + std::to_string(R) + (adj ? "_adj" : ""), (double)pk_bytes, R, adj != 0, {}});
  for (int round = -1; round < rounds; ++round) {       // round -1: warm-up, not recorded
    for (size_t v = 0; v < vars.size(); ++v) {
      CK(hipEventRecord(e0v, st));
      for (int i = 0; i < iters; ++i) {
        if (v == 0) run_loads_raw(); else if (v == 1) run_loads_pack(); else if (v == 2) run_raw(); else if (v == 3) run_packed();
        else launch_rows(vars[v].R, vars[v].adj);
      }
      CK(hipEventRecord(e1v, st));
      CK(hipEventSynchronize(e1v));
      float ms;
      CK(hipEventElapsedTime(&ms, e0v, e1v));
      if (round >= 0) vars[v].us.push_back(ms * 1e3 / iters);
    }
  }
  for (auto& v : vars) {
    printf("%-12s rounds:", v.name.c_str());             // in the order taken: an outlier round shows in every variant or in one
    for (double t : v.us) printf(" %.1f", t);
    printf("\n");
    std::sort(v.us.begin(), v.us.end());
    const double med = v.us[v.us.size() / 2];
    printf("%-12s us/pass min %.1f med %.1f max %.1f   %.0f GB/s own bytes (%.1f%% of 8 TB/s)\n", v.name.c_str(), v.us.front(), med,
           v.us.back(), v.bytes / (med * 1e-6) / 1e9, v.bytes / (med * 1e-6) / 8e12 * 100);
  }
  const double mr = vars[2].us[vars[2].us.size() / 2], mp = vars[3].us[vars[3].us.size() / 2];
  printf("packed_body / raw_body median time %.4f  (bytes ratio 0.8750; raw spread %.4f, packed spread %.4f of median)\n", mp / mr,
         (vars[2].us.back() - vars[2].us.front()) / mr, (vars[3].us.back() - vars[3].us.front()) / mp);
  // stop rule: a rows variant counts only if its median beats packed_body's by 5 x packed_body's own max - min
  const double spread = vars[3].us.back() - vars[3].us.front();
  for (size_t v = 4; v < vars.size(); ++v) {
    const double med = vars[v].us[vars[v].us.size() / 2];
    printf("%-12s / packed_body %.4f  / raw_body %.4f  gain %.1f us = %.1f x packed_body spread (%.1f us): %s\n", vars[v].name.c_str(),
           med / mp, med / mr, mp - med, spread > 0 ? (mp - med) / spread : 0.0, spread, mp - med >= 5 * spread ? "PASS" : "no");
  }
  for (void* q : {(void*)A, (void*)P, (void*)b, (void*)rout, (void*)y, (void*)rvec, (void*)slabs, (void*)g, (void*)gref, (void*)rr,
                  (void*)counts, (void*)row_cnt})
    CK(hipFree(q));
  return 0;
}

int main(int argc, char** argv) {
  const int64_t m = argc > 1 ? atoll(argv[1]) : 131072;
  const int iters = argc > 2 ? atoi(argv[2]) : 10;
  const int rounds = argc > 3 ? atoi(argv[3]) : 7;
  const int n = argc > 4 ? atoi(argv[4]) : 16384;
  if (m < 1 || iters < 1 || rounds < 1 || (n != 16384 && n != 8192)) { fprintf(stderr, "usage: packed_probe [m] [iters] [rounds] [16384|8192]\n"); return 2; }
  return n == 16384 ? run<1024>(m, iters, rounds) : run<512>(m, iters, rounds);
}
