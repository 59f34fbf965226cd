// libfos_hip.so, translation unit 1 of 4 - planner, kernel menus and the problem-level entry points of the C ABI
// (include/fos.h).  Host code only decides launch geometry and enqueues kernels; there is no CPU compute fallback.
#include "fos_internal.hpp"
#include "softmax_link.hpp"
#include "pointwise_link.hpp"
#include "gemv_packed.hpp"

namespace fosapi {

thread_local std::string g_err;


// ---- fused-kernel menu -------------------------------------------------------------------------------

template <typename T, int THREADS, int K, int R, int MINW, bool WITH_G, int NBUF, bool DUAL, bool DRAIN = false, bool CB = false,
          bool IL = false>
void fused_launch(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw, float* slabs,
                  double* rr_part, double* rr2_part, int nwg, hipStream_t st) {
  hipLaunchKernelGGL((fos::gemv_pair_kernel<T, THREADS, K, R, true, MINW, WITH_G, NBUF, IL, DUAL, DRAIN, float, false, CB>), dim3(nwg),
                     dim3(THREADS), 0, st, reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs, rr_part,
                     rr2_part);
}

// fp64-accumulating form (fos_gemv_pair_dd): y and the slabs are doubles

// Dynamic shared memory above the 64 KiB default has to be granted per kernel AND per device (the attribute lives in
// the device's code object); a bitmask of devices already served, updated atomically, keeps this thread-safe.
template <typename K>
int raise_dynamic_lds(K kernel, size_t bytes, std::atomic<uint64_t>& done) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return FOS_ERR_HIP;
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return FOS_OK;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
      hipSuccess)
    return FOS_ERR_HIP;
  done.fetch_or(bit, std::memory_order_release);
  return FOS_OK;
}

template <typename T, int THREADS, int K, int R, int MINW, bool YLDS, int NB = 2, bool IL = false, bool KEEPCVT = false>
void fused_launch_dd(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw, double* slabs,
                     double* rr_part, int nwg, hipStream_t st) {
  auto kern = fos::gemv_pair_kernel<T, THREADS, K, R, true, MINW, true, NB, IL, false, false, double, YLDS, false, false, KEEPCVT>;
  constexpr size_t lds = YLDS ? (size_t)THREADS * K * fos::ElemTraits<T>::EPC * sizeof(double) : 0;
  if constexpr (lds > 65536) {
    static std::atomic<uint64_t> done{0};
    (void)raise_dynamic_lds(kern, lds, done);       // on failure the launch below fails and LAUNCH_CHECK reports it
  }
  hipLaunchKernelGGL(kern, dim3(nwg), dim3(THREADS), lds, st, reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs,
                     rr_part, (double*)nullptr);
}



// three register tiles in flight where that measured faster (same-run ratio to the fp32 kernel, tools/bench_dd.py:
// (512,4) fp32 0.96 -> 0.99, bf16 (256,4) 0.77 -> 0.83, bf16 (512,4) 0.77 -> 0.80; the 256-thread fp32 geometries lost
// 2-3 % and the (512,8) fp32 geometry would spill: those keep two)
#define DD_ENTRY(DT, T, TH, K, R, YL) { DT, TH, K, R, fused_launch_dd<T, TH, K, R, 2, YL, 2> }
#define DD_ENTRY3(DT, T, TH, K, R, YL) { DT, TH, K, R, fused_launch_dd<T, TH, K, R, 2, YL, 3> }
#define DD_ENTRY_IL(DT, T, TH, K, R, YL) { DT, TH, K, R, fused_launch_dd<T, TH, K, R, 2, YL, 2>, fused_launch_dd<T, TH, K, R, 2, YL, 2, true> }
#define DD_ENTRY3_IL(DT, T, TH, K, R, YL) { DT, TH, K, R, fused_launch_dd<T, TH, K, R, 2, YL, 3>, fused_launch_dd<T, TH, K, R, 2, YL, 3, true> }
const DdEntry kDdMenu[] = {
    DD_ENTRY(FOS_F32, float, 64, 1, 4, false), DD_ENTRY(FOS_F32, float, 64, 2, 2, false),
    DD_ENTRY(FOS_F32, float, 64, 3, 2, false),             // 513..768 columns (on 256 x 1 at 62-75 % filled: 58-66 % of 8 TB/s)
    DD_ENTRY(FOS_F32, float, 256, 1, 2, false), DD_ENTRY(FOS_F32, float, 256, 2, 2, false),
    DD_ENTRY(FOS_F32, float, 256, 3, 1, false),            // (3, 5 chunks: widths between the powers of two, as in kMenu: +3-5 %)
    DD_ENTRY_IL(FOS_F32, float, 256, 4, 1, false), DD_ENTRY_IL(FOS_F32, float, 512, 3, 1, false),
    DD_ENTRY3_IL(FOS_F32, float, 512, 4, 1, false), DD_ENTRY_IL(FOS_F32, float, 512, 5, 1, false),
    DD_ENTRY_IL(FOS_F32, float, 512, 8, 1, true),          // (512 x 6 with y in LDS measured 3 % behind this one at 12288 columns)
    DD_ENTRY(FOS_BF16, fos::bf16_t, 64, 1, 2, false), DD_ENTRY(FOS_BF16, fos::bf16_t, 64, 2, 2, false),
    DD_ENTRY(FOS_BF16, fos::bf16_t, 256, 1, 2, false),
    DD_ENTRY(FOS_BF16, fos::bf16_t, 256, 2, 1, false), DD_ENTRY_IL(FOS_BF16, fos::bf16_t, 256, 3, 1, false),
    // bf16 rows of 4 chunks per thread: the pass is VALU-bound (56 VALU instructions per 16-byte chunk: unpack + convert
    // for the dot, AGAIN for the gradient update, 16 v_fma_f64), so these keep the converted tile across the barrier
    // (KEEPCVT: 40 instructions) and pay with registers - two tiles in flight instead of three, per-chunk scheduling
    // barriers, the cross-wave sum through the DPP ladder.  tools/dd_bench: 262144 x 8192 69.5 -> 78.2 % of 8 TB/s,
    // 131072 x 16384 66.6 -> 74.5 %.
    { FOS_BF16, 256, 4, 1, fused_launch_dd<fos::bf16_t, 256, 4, 1, 2, true, 2, false, true>,
      fused_launch_dd<fos::bf16_t, 256, 4, 1, 2, true, 2, true, true> },
    DD_ENTRY_IL(FOS_BF16, fos::bf16_t, 512, 3, 1, false),
    { FOS_BF16, 512, 4, 1, fused_launch_dd<fos::bf16_t, 512, 4, 1, 2, true, 2, false, true>,
      fused_launch_dd<fos::bf16_t, 512, 4, 1, 2, true, 2, true, true> },
};
#undef DD_ENTRY
#undef DD_ENTRY3
#undef DD_ENTRY_IL
#undef DD_ENTRY3_IL
// with-gradient / residual-only pair of a geometry: NB register tiles, drained or not, column-block (CB) or interleaved (IL)
#define PAIR(T, TH, K, R, W, NB, DRAIN, CB, IL) \
  fused_launch<T, TH, K, R, W, true, NB, false, DRAIN, CB, IL>, fused_launch<T, TH, K, R, W, false, NB, false, DRAIN, CB, IL>
// Every entry carries the column-block pair: a COLUMN-SHARDED problem (fos_problem_set_comm_cols) runs the two-phase
// plan at whatever width a rank's block has; the unsharded planner only ever lands on the two widest geometries.
#define ENTRY(DT, T, TH, K, R, W) \
  { DT, TH, K, R, PAIR(T, TH, K, R, W, 2, false, false, false), nullptr, nullptr, PAIR(T, TH, K, R, W, 2, false, true, false) }
// D: with DUAL
#define ENTRY_D(DT, T, TH, K, R, W) \
  { DT, TH, K, R, PAIR(T, TH, K, R, W, 2, false, false, false), fused_launch<T, TH, K, R, W, true, 2, true>, nullptr, \
    PAIR(T, TH, K, R, W, 2, false, true, false) }
// NB register tiles in flight (profiles/r01_kbench_exp_*.log: 3 tiles are worth 1.5 % at n = 8192) + DUAL + the
// interleaved-rows forms (rows >= 16 KiB)
#define ENTRY_NB_IL(DT, T, TH, K, R, W, NB) \
  { DT, TH, K, R, PAIR(T, TH, K, R, W, NB, false, false, false), fused_launch<T, TH, K, R, W, true, 2, true>, nullptr, \
    PAIR(T, TH, K, R, W, NB, false, true, false), PAIR(T, TH, K, R, W, NB, false, false, true), \
    fused_launch<T, TH, K, R, W, true, 2, true, false, false, true> }
// drained pipeline (profiles/r01_kbench_exp2_*: best form for 64 KiB rows), with DUAL
// The DUAL pass of such an entry runs another geometry of the same row step R (the 1024-thread form has no registers
// left for the second vector): TH2 x K2 must cover the same n.
#define ENTRY_DRAIN(DT, T, TH, K, R, W, TH2, K2, W2) \
  { DT, TH, K, R, PAIR(T, TH, K, R, W, 2, true, false, false), fused_launch<T, TH2, K2, R, W2, true, 2, true, false>, nullptr, \
    PAIR(T, TH, K, R, W, 2, true, true, false), PAIR(T, TH, K, R, W, 2, true, false, true), \
    fused_launch<T, TH2, K2, R, W2, true, 2, true, false, false, true> }
// Ordered by capacity (threads*k*EPC columns); first entry that fits n is the default.
// The 64-thread entries give narrow rows (65..512 columns) one WAVE per row instead of a 256-thread workgroup whose
// lanes would mostly idle (200000 x 256 ran at 18 % of the roofline on the 256-thread geometry); they are launched
// with proportionally more workgroups (plan_fused).
// Three-chunk geometries (round 3): a chunk beyond n is not idle - it re-reads the thread's chunk 0 to keep the loads
// branch-free - so a width of 3 * 2^k columns on the next power-of-two geometry paid for a quarter more load instructions
// (fp32 12288 columns 75 %, 10240 70 % of 8 TB/s against 84 % at 16384: tools/bench_widths.py).  Capacities are now
// 1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16 x 1024 columns (fp32), so from 2048 columns on at least 4/5 of the issued loads are
// live at any width (n = 5000 and 10000 land on the five-chunk geometries at 98 %).
// bf16 rows of 16385 ... 24576 columns get 512 threads x 6 chunks (1024 threads at 128 VGPRs spill; 8 chunks - y and the
// gradient slice 64 VGPRs each - spill at 256), 24577 ... 32768 the y-in-LDS kernel (gemv_wide.hpp), instead of two passes in
// column blocks (36 % of the roofline -> a single read).
#define ENTRY_IL_ND(DT, T, TH, K, R, W) \
  { DT, TH, K, R, PAIR(T, TH, K, R, W, 2, false, false, false), nullptr, nullptr, \
    PAIR(T, TH, K, R, W, 2, false, true, false), PAIR(T, TH, K, R, W, 2, false, false, true), nullptr }
const MenuEntry kMenu[] = {
    ENTRY_D(FOS_F32, float, 64, 1, 4, 2), ENTRY_D(FOS_F32, float, 64, 2, 4, 2),
    ENTRY_D(FOS_F32, float, 256, 1, 4, 2), ENTRY_D(FOS_F32, float, 256, 2, 4, 2), ENTRY_D(FOS_F32, float, 256, 3, 2, 2),
    ENTRY_D(FOS_F32, float, 256, 4, 2, 2), ENTRY_NB_IL(FOS_F32, float, 256, 5, 2, 2, 2),
    ENTRY_NB_IL(FOS_F32, float, 512, 3, 1, 2, 3),   ENTRY_NB_IL(FOS_F32, float, 512, 4, 1, 2, 3),
    ENTRY_NB_IL(FOS_F32, float, 512, 5, 1, 2, 3),   ENTRY_DRAIN(FOS_F32, float, 1024, 3, 1, 4, 512, 6, 2),
    ENTRY_NB_IL(FOS_F32, float, 512, 7, 1, 2, 2),   ENTRY_DRAIN(FOS_F32, float, 1024, 4, 1, 4, 512, 8, 2),
    ENTRY_D(FOS_F32, float, 512, 8, 1, 2),  ENTRY(FOS_F32, float, 1024, 2, 2, 4),
    ENTRY(FOS_BF16, fos::bf16_t, 64, 1, 4, 2), ENTRY(FOS_BF16, fos::bf16_t, 64, 2, 4, 2),   // one wave per row: up to 512 / 1024 bf16 columns
    ENTRY(FOS_BF16, fos::bf16_t, 256, 1, 4, 2), ENTRY(FOS_BF16, fos::bf16_t, 256, 2, 2, 2),
    ENTRY_NB_IL(FOS_BF16, fos::bf16_t, 256, 3, 1, 2, 3), ENTRY_NB_IL(FOS_BF16, fos::bf16_t, 256, 4, 1, 2, 3),
    ENTRY_IL_ND(FOS_BF16, fos::bf16_t, 256, 5, 1, 2),
    ENTRY_NB_IL(FOS_BF16, fos::bf16_t, 512, 3, 1, 2, 3), ENTRY_NB_IL(FOS_BF16, fos::bf16_t, 512, 4, 1, 2, 3),
    ENTRY_IL_ND(FOS_BF16, fos::bf16_t, 512, 5, 1, 2), ENTRY_IL_ND(FOS_BF16, fos::bf16_t, 512, 6, 1, 2),
};

const MenuEntry* find_entry(int dtype, int threads, int k, int r) {
  for (const auto& e : kMenu)
    if (e.dtype == dtype && e.threads == threads && e.k == k && e.r == r) return &e;
  return nullptr;
}
int epc_of(int dtype) { return dtype == FOS_F32 ? 4 : 8; }
// chunk-per-lane rows: up to 32 lanes per row - 128 fp32 / 256 bf16 columns
int64_t tlr_max_n(int dtype) { return 32 * (int64_t)epc_of(dtype); }
const MenuEntry* default_entry(int dtype, int64_t n) {
  for (const auto& e : kMenu)
    if (e.dtype == dtype && (int64_t)e.threads * e.k * epc_of(dtype) >= n) return &e;
  return nullptr;
}

// ---- wide rows (gemv_wide.hpp): y in LDS (dynamic shared memory above the 64 KiB default): 16384 < n <= 32768 fp32,
// 24576 < n <= 32768 bf16 ---
template <bool WITH_G, typename T>
void wide_launch(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw, float* slabs,
                 double* rr_part, double* /*rr2_part*/, int nwg, hipStream_t st) {
  static std::atomic<uint64_t> done{0};
  (void)raise_dynamic_lds(&fos::gemv_wide_kernel<WITH_G, T>, fos::WD_MAX_N * sizeof(float), done);   // failure: see LAUNCH_CHECK
  hipLaunchKernelGGL((fos::gemv_wide_kernel<WITH_G, T>), dim3(nwg), dim3(fos::WD_THREADS), (size_t)n * sizeof(float), st,
                     reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs, rr_part);
}
const MenuEntry kWideF32 = {FOS_F32, fos::WD_THREADS, fos::WD_K, 1, wide_launch<true, float>, wide_launch<false, float>, nullptr};
const MenuEntry kWideBf16 = {FOS_BF16, fos::WD_THREADS, fos::WD_K / 2, 1, wide_launch<true, fos::bf16_t>,
                             wide_launch<false, fos::bf16_t>, nullptr};
const MenuEntry* wide_entry(int dtype) { return dtype == FOS_F32 ? &kWideF32 : &kWideBf16; }

// ---- tall-skinny entries (gemv_tall.hpp): n <= 64, any m / lda; one entry per column capacity and load form --------
template <typename T, int NC, int LOAD, bool WITH_G, bool DUAL>
void tall_launch(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw, float* slabs,
                 double* rr_part, double* rr2_part, int nwg, hipStream_t st) {
  // The staged float4 copy streams one contiguous span: non-temporal once the matrix outgrows the 256 MiB Infinity Cache
  // (32000000 x 5: 71.8 -> 82.2 % of 8 TB/s); below that the cached form keeps the re-reads of a solver loop in the
  // cache (8000000 x 5 = 160 MB: 32.9 us cached, 34.7 us non-temporal).  tools/tall_bench.
  if (LOAD == fos::TL_STAGE4 && m * (int64_t)n * (int64_t)sizeof(T) > (192ll << 20))
    hipLaunchKernelGGL((fos::gemv_tall_kernel<T, NC, LOAD, WITH_G, DUAL, float, LOAD == fos::TL_STAGE4>), dim3(nwg),
                       dim3(fos::TL_THREADS), 0, st, reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs, rr_part, rr2_part);
  else
    hipLaunchKernelGGL((fos::gemv_tall_kernel<T, NC, LOAD, WITH_G, DUAL, float, false>), dim3(nwg), dim3(fos::TL_THREADS), 0, st,
                       reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs, rr_part, rr2_part);
}
template <typename T, int NC, int LOAD>
void tall_launch_dd(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw, double* slabs,
                    double* rr_part, int nwg, hipStream_t st) {
  if (LOAD == fos::TL_STAGE4 && m * (int64_t)n * (int64_t)sizeof(T) > (192ll << 20))
    hipLaunchKernelGGL((fos::gemv_tall_kernel<T, NC, LOAD, true, false, double, LOAD == fos::TL_STAGE4>), dim3(nwg),
                       dim3(fos::TL_THREADS), 0, st, reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs, rr_part, (double*)nullptr);
  else
    hipLaunchKernelGGL((fos::gemv_tall_kernel<T, NC, LOAD, true, false, double, false>), dim3(nwg), dim3(fos::TL_THREADS), 0, st,
                       reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs, rr_part, (double*)nullptr);
}
template <typename T, bool VEC>
void tallq_launch_dd(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw, double* slabs,
                     double* rr_part, int nwg, hipStream_t st) {
  hipLaunchKernelGGL((fos::gemv_tall_quad_kernel<T, VEC, true, false, double>), dim3(nwg), dim3(fos::TL_THREADS), 0, st,
                     reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs, rr_part, (double*)nullptr);
}
template <typename T, bool VEC, bool WITH_G, bool DUAL>
void tallq_launch(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw, float* slabs,
                  double* rr_part, double* rr2_part, int nwg, hipStream_t st) {
  hipLaunchKernelGGL((fos::gemv_tall_quad_kernel<T, VEC, WITH_G, DUAL>), dim3(nwg), dim3(fos::TL_THREADS), 0, st,
                     reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs, rr_part, rr2_part);
}
template <typename T, int LPR, bool WITH_G, bool DUAL>
void tallr_launch(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw, float* slabs,
                  double* rr_part, double* rr2_part, int nwg, hipStream_t st) {
  // fp32 pass: bf16 storage accumulates in fp32 like its streaming siblings, fp32 storage in fp64 (gemv_tall.hpp "AT")
  // (fp32 rows of 65..128 columns - 32 lanes per row - ran on the fp32-accumulating streaming kernel until round 3: fp32 too)
  using AT = typename std::conditional<std::is_same<T, float>::value && (LPR < 32), double, float>::type;
  hipLaunchKernelGGL((fos::gemv_tall_rows_kernel<T, LPR, WITH_G, DUAL, float, AT>), dim3(nwg), dim3(fos::TL_THREADS), 0, st,
                     reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs, rr_part, rr2_part);
}
template <typename T, int LPR>
void tallr_launch_dd(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw, double* slabs,
                     double* rr_part, int nwg, hipStream_t st) {
  hipLaunchKernelGGL((fos::gemv_tall_rows_kernel<T, LPR, true, false, double>), dim3(nwg), dim3(fos::TL_THREADS), 0, st,
                     reinterpret_cast<const T*>(A), lda, b, m, n, ys, rpw, slabs, rr_part, (double*)nullptr);
}
// aligned rows: a row per LPR lanes, one 16-byte chunk per lane (gemv_tall_rows_kernel); k = LPR marks the entry
#define TALLR(DT, T, LPR) \
  { DT, fos::TL_THREADS, LPR, 0, tallr_launch<T, LPR, true, false>, tallr_launch<T, LPR, false, false>, \
    tallr_launch<T, LPR, true, true>, tallr_launch_dd<T, LPR> }
// (a row per 4 lanes - up to 4 chunks - measured slower than the row-per-thread form and is not instantiated)
const MenuEntry kTallRowsF32[3] = {TALLR(FOS_F32, float, 8), TALLR(FOS_F32, float, 16), TALLR(FOS_F32, float, 32)};
const MenuEntry kTallRowsBf16[3] = {TALLR(FOS_BF16, fos::bf16_t, 8), TALLR(FOS_BF16, fos::bf16_t, 16), TALLR(FOS_BF16, fos::bf16_t, 32)};
#undef TALLR
// 33..64 columns: a row per quad of lanes (gemv_tall_quad_kernel)
#define TALLQ(DT, T, VEC) \
  { DT, fos::TL_THREADS, 0, 0, tallq_launch<T, VEC, true, false>, tallq_launch<T, VEC, false, false>, \
    tallq_launch<T, VEC, true, true>, tallq_launch_dd<T, VEC> }
#define TALL(DT, T, NC, LD) \
  { DT, fos::TL_THREADS, 0, 0, tall_launch<T, NC, LD, true, false>, tall_launch<T, NC, LD, false, false>, \
    tall_launch<T, NC, LD, true, true>, tall_launch_dd<T, NC, LD> }
#define TALL_ROW(DT, T, NC) \
  { TALL(DT, T, NC, fos::TL_DIRECT), TALL(DT, T, NC, fos::TL_VEC), TALL(DT, T, NC, fos::TL_STAGE), TALL(DT, T, NC, fos::TL_STAGE4) }
const MenuEntry kTallF32[4][4] = {
    TALL_ROW(FOS_F32, float, 8), TALL_ROW(FOS_F32, float, 16), TALL_ROW(FOS_F32, float, 32),
    {TALLQ(FOS_F32, float, false), TALLQ(FOS_F32, float, true), TALLQ(FOS_F32, float, false), TALLQ(FOS_F32, float, false)}};
const MenuEntry kTallBf16[4][2] = {
    {TALL(FOS_BF16, fos::bf16_t, 8, fos::TL_DIRECT), TALL(FOS_BF16, fos::bf16_t, 8, fos::TL_STAGE)},
    {TALL(FOS_BF16, fos::bf16_t, 16, fos::TL_DIRECT), TALL(FOS_BF16, fos::bf16_t, 16, fos::TL_STAGE)},
    {TALL(FOS_BF16, fos::bf16_t, 32, fos::TL_DIRECT), TALL(FOS_BF16, fos::bf16_t, 32, fos::TL_STAGE)},
    {TALLQ(FOS_BF16, fos::bf16_t, false), TALLQ(FOS_BF16, fos::bf16_t, false)}};
#undef TALL
#undef TALL_ROW
#undef TALLQ
// load form: 16-byte row loads when the layout allows, LDS staging for contiguous ragged matrices, scalar loads otherwise
const MenuEntry* tall_entry(int dtype, int64_t n, int64_t lda, const void* A) {
  const int epc = dtype == FOS_F32 ? 4 : 8;
  // Rows of 5..16 chunks of 16 bytes (fp32: 17..64 columns, bf16: 33..64): a row per 8 / 16 lanes, one chunk per lane
  // (4000000 x 32: 52 % -> 74 % of the roofline, 2000000 x 64: 53 % -> 73 %).  Up to 4 chunks the row-per-thread form
  // with 16-byte loads is the faster one (4000000 x 16: 72-76 % against 67-69 %, profiles/r02_sweep_wgs.log).
  if (n % epc == 0 && lda % epc == 0 && (reinterpret_cast<uintptr_t>(A) & 15u) == 0 && n / epc > 4) {
    // (round 3) 65..128 columns: a row per 32 lanes (fp32) / 16 lanes (bf16) - on the one-wave-per-row streaming geometry
    // a 72-column row left 46 of 64 lanes re-reading chunk 0 (53 % of 8 TB/s at 7456512 x 72; tools/bench_widths.py narrow)
    const int chunks = (int)(n / epc);
    if (dtype == FOS_F32) return &kTallRowsF32[chunks <= 8 ? 0 : chunks <= 16 ? 1 : 2];
    return &kTallRowsBf16[chunks <= 8 ? 0 : chunks <= 16 ? 1 : 2];       // bf16: up to 256 columns
  }
  const int idx = n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : 3;
  const bool contiguous = (lda == n);
  if (dtype == FOS_F32) {
    const bool vec = n % 4 == 0 && lda % 4 == 0 && (reinterpret_cast<uintptr_t>(A) & 15u) == 0;
    // contiguous ragged rows: staged through LDS; float4 copy when the matrix is 16-byte aligned (plan_tall keeps the
    // rows per workgroup a multiple of 4, so every block then starts on a 16-byte boundary)
    const bool a16 = (reinterpret_cast<uintptr_t>(A) & 15u) == 0;
    return &kTallF32[idx][vec ? fos::TL_VEC : (contiguous ? (a16 && idx < 3 ? fos::TL_STAGE4 : fos::TL_STAGE) : fos::TL_DIRECT)];
  }
  return &kTallBf16[idx][contiguous ? 1 : 0];
}

int grid_1d(int64_t n, int per_block, int cap) {
  int64_t g = (n + per_block - 1) / per_block;
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, cap));
}


void plan_fused(fos_problem* p, const MenuEntry* e, int nwg_hint) {
  p->pass.entry = e;
  p->pass.path = 0;
  int64_t m = p->m;
  // Workgroups per CU (profiles/r02_sweep_wgs.log): one for the wide geometries, whose register tiles already hold
  // 64-96 KiB of rows in flight per CU; two for the 256-thread geometries with 1-2 chunks per thread (1048576 x 1024:
  // 67 % -> 88 % of the roofline - one such workgroup has 32 KiB in flight, below HBM latency x bandwidth per CU);
  // 16 single-wave workgroups for the one-wave-per-row geometries.
  // One-wave-per-row geometries (64 threads), round 3: FOUR workgroups per CU - a wave per SIMD - not sixteen.  Whole step at
  // ~2 GiB (tools/wg_sweep.py, profiles/r03_wg_sweep.txt): 2097152 x 256 77.5 -> 86.1 % of 8 TB/s, 1048576 x 512 75.6 -> 84.3 %,
  // 1398016 x 320 71.2 -> 82.3 %; the A pass itself is 5-8 % faster with fewer, longer streams, and the update kernel sums a
  // quarter of the slabs (200000 x 256: its share fell from 26 to 8 us of a 63 -> 44 us iteration).  Rows that leave more than
  // a fifth of the wave's lanes without a chunk (n <= 204 on the one-chunk geometry) need eight: 2796032 x 160 74.3 -> 79.9 %.
  const bool sparse_wave = e->threads == 64 && e->k == 1 && p->n * 5 <= 4 * 64 * (int64_t)epc_of(p->dtype);
  // 256 threads: two per CU up to two chunks per thread, one above; a row that leaves lanes without a chunk wants one more -
  // 838656 x 640 on 256 x 1 (62 % filled): 77.5 -> 82.4 % with three, 209664 x 2560 on 256 x 3 (83 %): 82.3 -> 86.1 % with two
  // (full rows on 256 x 3: 88 % with one, 82 % with two)
  const int64_t cap256 = 256 * (int64_t)e->k * epc_of(p->dtype);
  const bool sparse_256 = e->threads == 256 && ((e->k == 1 && p->n * 10 <= 7 * cap256) || (e->k == 3 && p->n * 10 <= 9 * cap256));
  const int per_cu = e->threads >= 512 ? 1 : e->threads == 256 ? (e->k <= 2 ? 2 : 1) + (sparse_256 ? 1 : 0) : (sparse_wave ? 8 : 4);
  int nwg = nwg_hint > 0 ? nwg_hint : p->ncu * per_cu;
  // at least 2 row steps and 32 KiB of rows per workgroup: below that the slab (one row of n floats per workgroup) and the
  // slab sums rival the rows they cover (20000 x 256: 26 -> 17.5 us per iteration at 32 rows, 4096 x 512 best at 16 rows,
  // 100000 x 128 at 49-98 rows: profiles/r02_sweep_mid.txt)
  const int64_t row_bytes = p->n * (p->dtype == FOS_F32 ? 4 : 2);
  const int64_t min_rows = std::max<int64_t>(2 * (int64_t)e->r, (32768 + row_bytes - 1) / row_bytes);
  if (m < (int64_t)nwg * min_rows) nwg = (int)std::max<int64_t>(1, m / min_rows);
  p->pass.rows_per_wg = (m + nwg - 1) / nwg;
  p->pass.nwg = (int)((m + p->pass.rows_per_wg - 1) / p->pass.rows_per_wg);
  p->pass.nslabs = p->pass.nwg;
}

// Row-per-thread pass: every thread gets at least 4 rows when m allows, at most 4 workgroups per CU.
void plan_tall(fos_problem* p, const MenuEntry* e) {
  p->pass.entry = e;
  p->pass.path = 0;
  p->pass.tall = true;
  p->pass.slab_stride = fos::tall_slab_stride((int)p->n);
  p->pass.vec4 = true;                    // padded slab rows: the float4 epilogues serve ragged n as well
  // 4 workgroups per CU for the row-per-thread forms (profiles/r02_sweep_wgs.log)
  // (round 3, whole-step sweep tools/wg_sweep.py: the chunk-per-lane form wants 2 workgroups per CU when its rows fill the
  //  lanes - 2000000 x 64: 102.7 -> 89.6 us, 4000000 x 32: 93.3 -> 89.5 us - and 4 when a fifth or more of them idle -
  //  2000000 x 96: 155.6 -> 148.3 us; eight only made the update kernel sum more slabs.  It also keeps its workgroup count
  //  up on shorter matrices - 384 rows per workgroup are enough: 300000 x 64 31.6 -> 25.7 us, 200000 x 100 43.7 -> 30.0 us.)
  const int64_t lane_cols = (int64_t)e->k * epc_of(p->dtype);            // k = lanes per row of the chunk-per-lane entries
  // (a row per 32 lanes, 8 rows per workgroup step: three - 4194304 x 128: 76.1 % at two, 80.0 % at three or four)
  const int per_cu = e->k > 0 ? (p->n * 5 <= 4 * lane_cols ? 4 : (e->k >= 32 ? 3 : 2)) : 4;
  const int64_t rows_min = e->k > 0 ? 384 : 4 * fos::TL_THREADS;
  // Short matrices are latency-bound: up to one workgroup per CU from 64 rows each, whatever rows_min says (20000 x 5: 13.0 ->
  // 10.9 us per iteration, 10000 x 100: 14.6 -> 11.6 us, 30000 x 100: 16.8 -> 13.1 us; profiles/r03_wg_sweep.txt)
  const int64_t by_rows = std::max<int64_t>(p->m / rows_min, std::min<int64_t>(p->ncu, p->m / 64));
  int64_t nwg = std::max<int64_t>(1, std::min<int64_t>(per_cu * (int64_t)p->ncu, by_rows));
  p->pass.rows_per_wg = ((p->m + nwg - 1) / nwg + 3) / 4 * 4;     // a multiple of 4 rows: 16-byte aligned block starts (staged copy)
  p->pass.nwg = (int)((p->m + p->pass.rows_per_wg - 1) / p->pass.rows_per_wg);
  p->pass.nslabs = p->pass.nwg;
}

void plan_fallback(fos_problem* p) {
  p->pass.entry = nullptr;
  p->pass.path = 1;
  int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(64, p->m / 64));
  p->pass.rows_per_wg = (p->m + chunks - 1) / chunks;
  p->pass.nslabs = (int)((p->m + p->pass.rows_per_wg - 1) / p->pass.rows_per_wg);
  p->pass.nwg = p->pass.nslabs;
  p->pass.resid_grid = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (p->m + 3) / 4));
}

int ensure_workspace(fos_problem* p) {
  PassPlan& w = p->pass;
  int rc = w.slabs.reserve((size_t)w.nslabs * (w.slab_stride ? w.slab_stride : p->n));
  if (rc) return rc;
  const int need_rr = std::max(std::max(w.nwg, w.colblock ? 256 : 1), std::max(w.resid_grid, 1));
  if ((rc = w.rr_part.reserve(need_rr)) || (rc = w.rr2_part.reserve(need_rr))) return rc;
  if (w.path == 1 && (rc = w.rvec.reserve(p->m))) return rc;
  if (w.colblock && !w.zeros) {
    if ((rc = w.rneg.reserve(p->m)) || (rc = w.zeros.reserve(w.cb_width))) return rc;
    HIP_TRY(hipMemset(w.zeros, 0, (size_t)w.cb_width * sizeof(float)));
  }
  return FOS_OK;
}

int prof_drain(fos_problem* p) {
  if (p->ev_used == 0) return FOS_OK;
  HIP_TRY(hipEventSynchronize(p->ev_pool[p->ev_used - 1]));
  for (size_t i = 0; i + 1 < p->ev_used; i += 2) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, p->ev_pool[i], p->ev_pool[i + 1]));
    p->prof_ms += ms;
    p->prof_launches += 1;
  }
  p->ev_used = 0;
  return FOS_OK;
}

int prof_mark(fos_problem* p, bool start) {
  if (!p->profiling) return FOS_OK;
  if (start) {
    p->prof_open = (p->prof_seq++ % p->profiling) == 0;
    if (!p->prof_open) return FOS_OK;
  } else if (!p->prof_open) {
    return FOS_OK;
  }
  if (start && p->ev_used + 2 > p->ev_pool.size()) {
    if (p->ev_pool.size() >= 8192) {          // bounded pool: fold what we have (synchronises)
      int rc = prof_drain(p);
      if (rc) return rc;
    } else {
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        p->ev_pool.push_back(e);
      }
    }
  }
  HIP_TRY(hipEventRecord(p->ev_pool[p->ev_used++], p->stream));
  return FOS_OK;
}

// Enqueue the A pass for `ys`.  with_g: also produce the slabs (A^T r).  Returns number of rr partials.
int launch_pass_inner(fos_problem* p, const YSource& ys, const float* b, bool with_g, int* n_rr, bool dual, double* rr_to);
int launch_pass(fos_problem* p, const YSource& ys, const float* b, bool with_g, int* n_rr, bool dual, double* rr_to) {
  int rc;
  // FOS_PLAN_PACK: the first with-gradient pass of ANY entry point packs (the planner's own choice waits for a FISTA run)
  if (p->pack_mode == 1 && !p->pk.tried && with_g && !dual && (rc = ensure_packed(p))) return rc;
  if ((rc = prof_mark(p, true))) return rc;
  if ((rc = launch_pass_inner(p, ys, b, with_g, n_rr, dual, rr_to))) return rc;
  return prof_mark(p, false);
}


__global__ __launch_bounds__(256) void sumsq_partials_kernel(const float* __restrict__ v, int64_t m, double* __restrict__ part,
                                                            const int* stopped) {
  if (stopped != nullptr && *stopped != 0) return;
  __shared__ double ws[4];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) acc += (double)v[i] * (double)v[i];
  acc = fos::wave_sum(acc);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

// v *= scale, only once the solver has stopped (column-sharded runs: keeps the in-place all-reduce of a no-op iteration
// from compounding; the values are not consumed any more, this only keeps them finite)
__global__ __launch_bounds__(256) void unsum_if_stopped_kernel(float* __restrict__ v, int64_t m, float scale, const int* stopped) {
  if (*stopped == 0) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) v[i] *= scale;
}

// The two-pass form (ragged / misaligned layouts, column-sharded fp64 pass), for the fp32 pass and the fp64 pass alike.
// Pass 1: r = A y - b into pass.rvec (fp64) and `grid` partials of ||r||^2 into rr.
int launch_residual_rows(fos_problem* p, const YSource& ys, const float* b, int grid, double* rr) {
  if (p->dtype == FOS_F32)
    hipLaunchKernelGGL(fos::residual_rows_kernel<float>, dim3(grid), dim3(256), 0, p->stream, (const float*)p->A, p->lda, b,
                       p->m, (int)p->n, ys, p->pass.rvec, rr);
  else
    hipLaunchKernelGGL(fos::residual_rows_kernel<fos::bf16_t>, dim3(grid), dim3(256), 0, p->stream, (const fos::bf16_t*)p->A,
                       p->lda, b, p->m, (int)p->n, ys, p->pass.rvec, rr);
  LAUNCH_CHECK();
  return FOS_OK;
}
// Pass 2: slab c = A[rows of chunk c]^T r, `chunks` chunks of rows_per_chunk rows, float or double slabs.
template <typename ACC>
int launch_transpose_rows(fos_problem* p, const int* stopped, int chunks, int64_t rows_per_chunk, ACC* slabs) {
  const dim3 grid((unsigned)((p->n + 255) / 256), (unsigned)chunks);
  if (p->dtype == FOS_F32)
    hipLaunchKernelGGL((fos::transpose_rows_kernel<float, ACC>), grid, dim3(256), 0, p->stream, (const float*)p->A, p->lda, p->m,
                       (int)p->n, p->pass.rvec, stopped, rows_per_chunk, slabs);
  else
    hipLaunchKernelGGL((fos::transpose_rows_kernel<fos::bf16_t, ACC>), grid, dim3(256), 0, p->stream, (const fos::bf16_t*)p->A,
                       p->lda, p->m, (int)p->n, p->pass.rvec, stopped, rows_per_chunk, slabs);
  LAUNCH_CHECK();
  return FOS_OK;
}

// Column blocks (rows wider than any single-pass kernel): phase 1 accumulates the negated residual block by block with the
// residual-only form of the streaming kernel, phase 2 is the SAME with-gradient kernel per block with y = 0 and b = -r
// (its row "dot" is then exactly r_i), writing its columns of full-width slabs.  A is read twice, at streaming speed.
int launch_pass_colblock(fos_problem* p, const YSource& ys, const float* b, bool with_g, int* n_rr) {
  const int64_t W = p->pass.cb_width, esz = p->dtype == FOS_F32 ? 4 : 2;
  const int nblk = (int)((p->n + W - 1) / W);
  const char* Ab = reinterpret_cast<const char*>(p->A);
  for (int cb = 0; cb < nblk; ++cb) {
    const int64_t c0 = cb * W;
    const int nb = (int)std::min<int64_t>(W, p->n - c0);
    YSource yb = ys;
    if (ys.y) yb.y = ys.y + c0;
    if (ys.x_cur) { yb.x_cur = ys.x_cur + c0; yb.x_prev = ys.x_prev + c0; }
    if (ys.yd) yb.yd = ys.yd + c0;
    yb.res_out = p->pass.rneg;
    yb.res_accum = cb > 0;
    // column-sharded: b enters the sum over the ranks once (rank 0)
    const float* b_here = (cb == 0 && !(p->col_sharded && p->comm->rank != 0)) ? b : nullptr;
    p->pass.entry->resid_only_cb(Ab + c0 * esz, p->lda, b_here, p->m, nb, yb, p->pass.rows_per_wg, p->pass.slabs, p->pass.rr2_part,
                            p->pass.rr2_part, p->pass.nwg, p->stream);
    LAUNCH_CHECK();
  }
  if (p->col_sharded) {              // r = sum over the column blocks of ALL ranks: the one m-vector exchange
    if (ys.stopped != nullptr) {     // after a stop the passes above were no-ops and rneg still holds the last SUM: divide
      hipLaunchKernelGGL(unsum_if_stopped_kernel, dim3(grid_1d(p->m, 256, 1024)), dim3(256), 0, p->stream, p->pass.rneg, p->m,   // it back
                         1.0f / (float)p->comm->nranks, ys.stopped);
      LAUNCH_CHECK();
    }
    int rc = reduce_across(p, p->pass.rneg, (size_t)p->m, false);
    if (rc) return rc;
  }
  if (!with_g) {
    hipLaunchKernelGGL(sumsq_partials_kernel, dim3(256), dim3(256), 0, p->stream, p->pass.rneg, p->m, p->pass.rr_part, ys.stopped);
    LAUNCH_CHECK();
    *n_rr = 256;
    return FOS_OK;
  }
  for (int cb = 0; cb < nblk; ++cb) {
    const int64_t c0 = cb * W;
    const int nb = (int)std::min<int64_t>(W, p->n - c0);
    YSource yz{p->pass.zeros, nullptr, nullptr, nullptr, ys.stopped};
    yz.slab_stride = p->n;
    p->pass.entry->with_g_cb(Ab + c0 * esz, p->lda, p->pass.rneg, p->m, nb, yz, p->pass.rows_per_wg, p->pass.slabs + c0, cb == 0 ? p->pass.rr_part : p->pass.rr2_part,
                        p->pass.rr2_part, p->pass.nwg, p->stream);
    LAUNCH_CHECK();
  }
  *n_rr = p->pass.nwg;
  return FOS_OK;
}

// ---- 28-bit packed copy of an fp32 A for the gradient pass (gemv_packed.hpp; PackPlan) ------------------------------------
// Where the planner packs without being asked (FOS_PLAN_PACK packs wherever the copy is served): the sweep in
// profiles/packed/README.md.  Rows of 8193 .. 16384 columns (the 1024-thread geometry) from 2 GiB on - the smallest size
// measured, ahead by 8-10 % there and at 4, 8, 16 and 64 GiB.  The 512-thread geometry (n <= 8192) measured 11-15 % BEHIND the
// raw pass with one row per drain and 3-10 % ahead with 4 rows per burst, but at 4 and 8 GiB by 1.6 times the raw pass's spread
// between repeats where the rule for moving this bound asks for 5 (a noisy run; README "Rows per burst"): still forced only.
constexpr int64_t PACK_MIN_BYTES = 2ll << 30;
constexpr int64_t PACK_MIN_N = 8193;
constexpr double PACK_MAX_EXCEPTIONS = 1e-3;       // share of out-of-window elements above which A stays raw

// Rows per burst of the packed pass (gemv_packed.hpp): the override of the last replan, else what the probe measured fastest
// for the geometry and row order (profiles/packed/README.md, "Rows per burst").  1024 threads: 3 with interleaved rows (64 GiB:
// 8454 us against 8492 with 2 and 8831 for one row per drain from two tiles), 2 with row blocks (8 GiB: 1053 / 1058 / 1067 us
// for 2 / 3 / one row).  512 threads: 4 at every size from 2 to 16 GiB, both row orders.
int pack_rows(const fos_problem* p) {
  if (p->pk.rows) return p->pk.rows;
  return p->n <= 8192 ? 4 : (p->il ? 3 : 2);
}

bool vec_layout(const fos_problem* p);
bool pack_served(const fos_problem* p) {
  const PassPlan& w = p->pass;
  return p->dtype == FOS_F32 && w.path == 0 && !w.tall && !w.colblock && !w.resident && !p->col_sharded && w.entry != nullptr &&
         w.entry != wide_entry(FOS_F32) && p->n % fos::pk::CPT == 0 && p->n <= 16384 && p->m < (1ll << 31) - 1 && vec_layout(p);
}

// first exponent (even) of the 16-binade window that holds most of hist[256]
unsigned pack_window(const int64_t (&hist)[256]) {
  unsigned best = 2;
  int64_t best_cnt = -1;
  for (unsigned e0 = 2; e0 <= fos::pk::E0_MAX; e0 += 2) {
    int64_t c = 0;
    for (unsigned e = e0; e < e0 + 16; ++e) c += hist[e];
    if (c > best_cnt) { best_cnt = c; best = e0; }
  }
  return best;
}

int ensure_packed(fos_problem* p) {
  namespace pk = fos::pk;
  PackPlan& k = p->pk;
  if (k.tried) return FOS_OK;
  k.tried = true;
  const int64_t m = p->m, n = p->n;
  if (p->pack_mode == 2 || !pack_served(p)) return FOS_OK;
  if (p->pack_mode == 0 && (m * n * 4 < PACK_MIN_BYTES || n < PACK_MIN_N)) return FOS_OK;
  const int threads = n <= 8192 ? 512 : 1024;
  const size_t p_bytes = (size_t)m * (size_t)pk::row_bytes(threads);
  HIP_TRY(hipStreamSynchronize(p->stream));
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  // the copy, the exception lists at their cap (8 values of 4 bytes each), the m-vectors, and a margin for the caller
  const size_t need = p_bytes + (size_t)((double)m * n * PACK_MAX_EXCEPTIONS) * 32 + (size_t)m * 16 + p_bytes / 16 + ((size_t)256 << 20);
  if (free_b < need) return FOS_OK;
  const float* A = static_cast<const float*>(p->A);

  // 1. window: exponent histogram of a sample of whole rows, on the host
  unsigned e0;
  {
    const int64_t srows = std::min<int64_t>(m, std::max<int64_t>(1, (4ll << 20) / n)), stride = m / srows;
    std::vector<float> sample((size_t)srows * n);
    HIP_TRY(hipMemcpy2D(sample.data(), (size_t)n * 4, A, (size_t)stride * p->lda * 4, (size_t)n * 4, (size_t)srows, hipMemcpyDeviceToHost));
    int64_t hist[256] = {0};
    for (float v : sample) {
      unsigned u;
      std::memcpy(&u, &v, 4);
      ++hist[(u >> 23) & 0xffu];
    }
    e0 = pack_window(hist);
  }
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((m * threads + 255) / 256, (int64_t)p->ncu * 32));
  auto refuse = [&]() { const int rows = k.rows; k.reset(); k.tried = true; k.rows = rows; return FOS_OK; };

  // 2. count the exceptions of every row (and look for inf / NaN): the CSR row pointers
  DevBuf<int> row_cnt;
  DevBuf<unsigned> flags;
  if (row_cnt.reserve((size_t)m) || flags.reserve(1)) return refuse();
  HIP_TRY(hipMemsetAsync(row_cnt, 0, (size_t)m * sizeof(int), p->stream));
  HIP_TRY(hipMemsetAsync(flags, 0, sizeof(unsigned), p->stream));
  hipLaunchKernelGGL(pk::pack_rows_kernel<true>, dim3(grid), dim3(256), 0, p->stream, A, p->lda, m, (int)n, threads, e0,
                     (unsigned char*)nullptr, row_cnt.get(), flags.get(), (const int*)nullptr, (int*)nullptr, (float*)nullptr,
                     (float*)nullptr);
  LAUNCH_CHECK();
  std::vector<int> ptr((size_t)m + 1);
  unsigned hflags = 0;
  HIP_TRY(hipMemcpyAsync(ptr.data() + 1, row_cnt, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipMemcpyAsync(&hflags, flags, sizeof(unsigned), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  if (hflags) return refuse();                                       // inf or NaN in A
  int64_t nnz = 0;
  ptr[0] = 0;
  for (int64_t i = 1; i <= m; ++i) {
    nnz += ptr[i];
    if (nnz > (1ll << 30)) return refuse();
    ptr[i] = (int)nnz;
  }
  if ((double)nnz > PACK_MAX_EXCEPTIONS * (double)m * (double)n) return refuse();

  // 3. pack; exceptions land in their row's segment in arrival order
  const size_t cap = (size_t)std::max<int64_t>(nnz, 1);
  if (k.P.reserve(p_bytes) || k.csr_ptr.reserve((size_t)m + 1) || k.csr_col.reserve(cap) || k.csr_tv.reserve(cap) ||
      k.csr_pv.reserve(cap) || k.csc_ptr.reserve((size_t)n + 1) || k.csc_row.reserve(cap) || k.csc_tv.reserve(cap) ||
      k.csc_pv.reserve(cap) || k.bprime.reserve((size_t)m) || k.r.reserve((size_t)m))
    return refuse();
  HIP_TRY(hipMemcpyAsync(k.csr_ptr, ptr.data(), ((size_t)m + 1) * sizeof(int), hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipMemsetAsync(row_cnt, 0, (size_t)m * sizeof(int), p->stream));
  hipLaunchKernelGGL(pk::pack_rows_kernel<false>, dim3(grid), dim3(256), 0, p->stream, A, p->lda, m, (int)n, threads, e0, k.P.get(),
                     row_cnt.get(), flags.get(), (const int*)k.csr_ptr.get(), k.csr_col.get(), k.csr_tv.get(), k.csr_pv.get());
  LAUNCH_CHECK();
  HIP_TRY(hipStreamSynchronize(p->stream));

  // 4. fixed order: columns ascending within a row, rows ascending within a column (the column-sorted copy)
  if (nnz > 0) {
    std::vector<int> col((size_t)nnz), row((size_t)nnz), perm;
    std::vector<float> tv((size_t)nnz), pv((size_t)nnz), tv2((size_t)nnz), pv2((size_t)nnz);
    std::vector<int> col2((size_t)nnz), cptr((size_t)n + 1, 0);
    HIP_TRY(hipMemcpy(col.data(), k.csr_col, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tv.data(), k.csr_tv, (size_t)nnz * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pv.data(), k.csr_pv, (size_t)nnz * sizeof(float), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < m; ++i) {
      const int lo = ptr[i], hi = ptr[i + 1];
      if (lo == hi) continue;
      perm.resize((size_t)(hi - lo));
      for (int q = lo; q < hi; ++q) perm[(size_t)(q - lo)] = q;
      std::sort(perm.begin(), perm.end(), [&](int a, int b) { return col[(size_t)a] < col[(size_t)b]; });
      for (int q = lo; q < hi; ++q) {
        const size_t src = (size_t)perm[(size_t)(q - lo)];
        col2[(size_t)q] = col[src]; tv2[(size_t)q] = tv[src]; pv2[(size_t)q] = pv[src];
        ++cptr[(size_t)col[src] + 1];
      }
    }
    for (int64_t j = 0; j < n; ++j) cptr[(size_t)j + 1] += cptr[(size_t)j];
    std::vector<int> fill(cptr.begin(), cptr.end() - 1);
    for (int64_t i = 0; i < m; ++i)
      for (int q = ptr[i]; q < ptr[i + 1]; ++q) {
        const size_t dst = (size_t)fill[(size_t)col2[(size_t)q]]++;
        row[dst] = (int)i; tv[dst] = tv2[(size_t)q]; pv[dst] = pv2[(size_t)q];
      }
    HIP_TRY(hipMemcpy(k.csr_col, col2.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k.csr_tv, tv2.data(), (size_t)nnz * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k.csr_pv, pv2.data(), (size_t)nnz * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k.csc_ptr, cptr.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k.csc_row, row.data(), (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k.csc_tv, tv.data(), (size_t)nnz * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k.csc_pv, pv.data(), (size_t)nnz * sizeof(float), hipMemcpyHostToDevice));
  }
  k.threads = threads;
  k.e0 = e0;
  k.nnz = nnz;
  k.active = true;
  return FOS_OK;
}

// The with-gradient pass from the packed copy: b' = b - D y, the pass on b' (stores r), slab 0 += D^T r.
int launch_pass_packed(fos_problem* p, const YSource& ys, const float* b, int* n_rr, double* rr_to) {
  namespace pk = fos::pk;
  PackPlan& k = p->pk;
  const float* bp = b;
  if (k.nnz > 0) {
    hipLaunchKernelGGL(pk::pk_bprime_kernel, dim3((unsigned)((p->m + 255) / 256)), dim3(256), 0, p->stream, (const int*)k.csr_ptr.get(),
                       (const int*)k.csr_col.get(), (const float*)k.csr_tv.get(), (const float*)k.csr_pv.get(), b, p->m, ys,
                       k.bprime.get());
    LAUNCH_CHECK();
    bp = k.bprime;
  }
  const int rows = pack_rows(p);
  auto pick = [&](auto il) {                 // instantiations kept, as probed: 1, 2, 3 rows at 1024 threads, 1 .. 4 at 512
    constexpr bool IL = decltype(il)::value;
    using Kern = decltype(&pk::gemv_packed_kernel<1024, IL, 1>);
    static const Kern menu[2][pk::MAX_ROWS] = {
        {pk::gemv_packed_kernel<512, IL, 1>, pk::gemv_packed_kernel<512, IL, 2>, pk::gemv_packed_kernel<512, IL, 3>,
         pk::gemv_packed_kernel<512, IL, 4>},
        {pk::gemv_packed_kernel<1024, IL, 1>, pk::gemv_packed_kernel<1024, IL, 2>, pk::gemv_packed_kernel<1024, IL, 3>, nullptr}};
    return menu[k.threads == 1024][rows - 1];
  };
  auto kern = p->il ? pick(std::true_type{}) : pick(std::false_type{});
  if (!kern) return fail(FOS_ERR_UNSUPPORTED, "packed pass: 4 rows per burst are not instantiated for the 1024-thread geometry");
  hipLaunchKernelGGL(kern, dim3(p->pass.nwg), dim3(k.threads), 0, p->stream, (const unsigned char*)k.P.get(), bp, p->m, (int)p->n, ys,
                     (k.e0 >> 1) * 0x01010101u, p->pass.rows_per_wg, p->pass.slabs.get(), k.r.get(),
                     rr_to ? rr_to : p->pass.rr_part.get());
  LAUNCH_CHECK();
  if (k.nnz > 0) {
    hipLaunchKernelGGL(pk::pk_dtr_kernel, dim3((unsigned)((p->n + 3) / 4)), dim3(256), 0, p->stream, (const int*)k.csc_ptr.get(),
                       (const int*)k.csc_row.get(), (const float*)k.csc_tv.get(), (const float*)k.csc_pv.get(), (const float*)k.r.get(),
                       (int)p->n, ys.stopped, p->pass.slabs.get());
    LAUNCH_CHECK();
  }
  *n_rr = p->pass.nwg;
  return FOS_OK;
}

int launch_pass_inner(fos_problem* p, const YSource& ys, const float* b, bool with_g, int* n_rr, bool dual, double* rr_to) {
  if (p->pass.path == 0 && p->pass.colblock) return launch_pass_colblock(p, ys, b, with_g, n_rr);
  if (p->pk.active && with_g && !dual) return launch_pass_packed(p, ys, b, n_rr, rr_to);
  if (p->pass.path == 0) {
    FusedLaunch fn = dual ? p->pass.entry->dual : (with_g ? p->pass.entry->with_g : p->pass.entry->resid_only);
    if (p->il) {
      FusedLaunch fi = dual ? p->pass.entry->dual_il : (with_g ? p->pass.entry->with_g_il : p->pass.entry->resid_only_il);
      if (fi) fn = fi;
    }
    fn(p->A, p->lda, b, p->m, (int)p->n, ys, p->pass.rows_per_wg, p->pass.slabs, rr_to && !dual ? rr_to : p->pass.rr_part.get(),
       rr_to && dual ? rr_to : p->pass.rr2_part.get(), p->pass.nwg, p->stream);
    LAUNCH_CHECK();
    *n_rr = p->pass.nwg;
    return FOS_OK;
  }
  int rc = launch_residual_rows(p, ys, b, p->pass.resid_grid, p->pass.rr_part);
  if (rc) return rc;
  *n_rr = p->pass.resid_grid;
  return with_g ? launch_transpose_rows<float>(p, ys.stopped, p->pass.nslabs, p->pass.rows_per_wg, p->pass.slabs.get()) : FOS_OK;
}


__global__ void rr_from_gbuf_kernel(const float* __restrict__ gbuf, int n, double* __restrict__ rr_out, const int* stopped) {
  if (stopped != nullptr && *stopped != 0) return;
  *rr_out = (double)gbuf[n];
}

int launch_slab_reduce_local(fos_problem* p, int n_rr, float* gbuf, double* rr_out, const int* stopped);
// slabs -> gbuf[0..n], summed over the ranks when the problem is sharded; rr_out (nullable) = the global ||r||^2
int launch_slab_reduce(fos_problem* p, int n_rr, float* gbuf, double* rr_out, const int* stopped) {
  if (!p->comm || p->col_sharded)                       // column-sharded: the gradient block is local, ||r||^2 already global
    return launch_slab_reduce_local(p, n_rr, gbuf, rr_out, stopped);
  // Row-sharded: gbuf is all-reduced IN PLACE, and the collective cannot be skipped on the device.  After a device-side
  // stop the A pass is a no-op and the slabs keep the last active iteration's partials, so the local sum is re-derived
  // from them UNCONDITIONALLY: every further enqueued iteration then all-reduces the same partials to the same sums (a
  // guarded no-op would leave the previous SUM in gbuf and the next all-reduce would multiply it by the number of ranks:
  // fp32 overflow after ~43 no-op iterations at 8 ranks).  rr_out is written after the exchange, guarded.
  int rc = launch_slab_reduce_local(p, n_rr, gbuf, nullptr, nullptr);
  if (rc) return rc;
  if ((rc = reduce_across(p, gbuf, (size_t)p->n + 1, false))) return rc;
  if (rr_out != nullptr) {
    hipLaunchKernelGGL(rr_from_gbuf_kernel, dim3(1), dim3(1), 0, p->stream, gbuf, (int)p->n, rr_out, stopped);
    LAUNCH_CHECK();
  }
  return FOS_OK;
}

int launch_slab_reduce_local(fos_problem* p, int n_rr, float* gbuf, double* rr_out, const int* stopped) {
  const int grid = (int)((p->n + fos::RCOLS - 1) / fos::RCOLS);
  if (p->pass.vec4)
    hipLaunchKernelGGL(fos::slab_reduce_kernel<true>, dim3(grid), dim3(256), 0, p->stream, p->pass.slabs, p->pass.nslabs,
                       (int)p->n, p->pass.rr_part, n_rr, gbuf, rr_out, stopped, p->pass.slab_stride);
  else
    hipLaunchKernelGGL(fos::slab_reduce_kernel<false>, dim3(grid), dim3(256), 0, p->stream, p->pass.slabs, p->pass.nslabs,
                       (int)p->n, p->pass.rr_part, n_rr, gbuf, rr_out, stopped);
  LAUNCH_CHECK();
  return FOS_OK;
}

__global__ void xp_pack_kernel(const float* __restrict__ X, int n, int n_pad, int nv, float* __restrict__ xp) {
  for (int col = blockIdx.x * 256 + threadIdx.x; col < n_pad; col += gridDim.x * 256)
    for (int j = 0; j < fos::BT_NV; ++j) xp[fos::xp_index(col, j)] = (col < n && j < nv) ? X[(int64_t)col * fos::BT_NV + j] : 0.f;
}

int ensure_batch_workspace(fos_problem* p) {
  if (p->cand.planned) return FOS_OK;
  const int64_t tile_cols = p->dtype == FOS_BF16 ? fos::BQ_COLS : fos::BT_COLS;
  p->cand.n_pad = (p->n + tile_cols - 1) / tile_cols * tile_cols;
  // fp32: Xp, one float per (column, candidate); bf16: Xq, three bf16 terms per (column, candidate)
  const size_t per_entry = p->dtype == FOS_BF16 ? 3 * sizeof(unsigned short) : sizeof(float);
  int rc;
  if ((rc = p->cand.xp.reserve((size_t)p->cand.n_pad * fos::BT_NV * per_entry / sizeof(float))) ||
      (rc = p->cand.q_part.reserve((size_t)(3 * p->ncu + 8) * fos::BT_NV)) || (rc = p->cand.bt_out.reserve(128)))
    return rc;
  p->cand.planned = true;
  return FOS_OK;
}

// The caller's X (n x 16 floats, row-major; columns 0..nv-1 used) -> the candidate block of product 1 (Xp, or Xq for bf16).
int pack_candidates(fos_problem* p, const float* X, int nv) {
  if (p->dtype == FOS_BF16)
    hipLaunchKernelGGL(fos::xq_pack_kernel, dim3(grid_1d(p->cand.n_pad, 256, 256)), dim3(256), 0, p->stream, X, (int)p->n,
                       (int)p->cand.n_pad, nv, (unsigned short*)p->cand.xp.get());
  else
    hipLaunchKernelGGL(xp_pack_kernel, dim3(grid_1d(p->cand.n_pad, 256, 256)), dim3(256), 0, p->stream, X, (int)p->n,
                       (int)p->cand.n_pad, nv, p->cand.xp);
  LAUNCH_CHECK();
  return FOS_OK;
}

// Product 1 (batch_trial.hpp): the kernel pointers stay typed, so every instantiation is checked against its signature.
typedef void (*Bf16Batch)(const fos::bf16_t*, int64_t, const float*, int, int64_t, int, const unsigned short*, int64_t, double*,
                          float*, const int*, const uint8_t*, fos::FoldHeld, const float*);
typedef void (*F32Batch)(const float*, int64_t, const float*, int, int64_t, int, const float*, int64_t, double*, float*,
                         const int*, const uint8_t*, fos::FoldHeld, const float*);

// The launchable forms of product 1, one line each: X(STORE_R, BBLOCK, FOLD, LOSS, WEIGHT).  STORE_R also keeps R
// (gram_batch.hpp reads it); BBLOCK: a right-hand side per column (B16 block); FOLD_TRAIN keeps R with every column zero on its
// held-out rows, FOLD_HELD sums over the held-out rows only (K-fold cross-validation in lockstep); LOSS_LOGISTIC: R =
// sigma(A Y) - b and the log-loss sums (b holds labels in [0, 1]); WEIGHT: R and the sums weighted per row
// (fos_row_weights_bind).  tests/_menu_product1.py reads this list and FOS_P1_ENTRY.
#define FOS_P1_FORMS(X)                                  \
  X(false, false, FOLD_OFF, LOSS_SQUARED, false)         \
  X(true, false, FOLD_OFF, LOSS_SQUARED, false)          \
  X(false, true, FOLD_OFF, LOSS_SQUARED, false)          \
  X(true, true, FOLD_OFF, LOSS_SQUARED, false)           \
  X(true, false, FOLD_TRAIN, LOSS_SQUARED, false)        \
  X(false, false, FOLD_HELD, LOSS_SQUARED, false)        \
  X(true, false, FOLD_OFF, LOSS_LOGISTIC, false)         \
  X(false, false, FOLD_OFF, LOSS_LOGISTIC, false)        \
  X(true, false, FOLD_TRAIN, LOSS_LOGISTIC, false)       \
  X(false, false, FOLD_HELD, LOSS_LOGISTIC, false)       \
  X(true, false, FOLD_OFF, LOSS_SQUARED, true)           \
  X(false, false, FOLD_OFF, LOSS_SQUARED, true)          \
  X(true, false, FOLD_TRAIN, LOSS_SQUARED, true)         \
  X(false, false, FOLD_HELD, LOSS_SQUARED, true)         \
  X(true, false, FOLD_OFF, LOSS_LOGISTIC, true)          \
  X(false, false, FOLD_OFF, LOSS_LOGISTIC, true)         \
  X(true, false, FOLD_TRAIN, LOSS_LOGISTIC, true)        \
  X(false, false, FOLD_HELD, LOSS_LOGISTIC, true)

// A form and the four kernels it stands for: fp32 and bf16 (column tile 128), each at RB 1 and RB 2 (index: tile variant).
struct BatchForm { bool store, bblock; int fold, loss; bool weight; };
struct BatchEntry { BatchForm form; F32Batch f32[2]; Bf16Batch bf16[2]; };
#define FOS_P1_ENTRY(S, B, F, L, W)                                                                                               \
  {{S, B, fos::F, fos::L, W},                                                                                                     \
   {fos::residual_batch_mfma_kernel<1, S, B, fos::F, fos::L, W>, fos::residual_batch_mfma_kernel<2, S, B, fos::F, fos::L, W>},    \
   {fos::residual_batch_mfma_bf16_kernel<1, 128, S, B, fos::F, fos::L, W>,                                                        \
    fos::residual_batch_mfma_bf16_kernel<2, 128, S, B, fos::F, fos::L, W>}},
const BatchEntry kBatchForms[] = {FOS_P1_FORMS(FOS_P1_ENTRY)};
#undef FOS_P1_ENTRY

// The two tile variants (row blocks per wave RB 1, 2): rows per workgroup, workgroups per CU for fp32 and for bf16.
// bf16, measured at 65536 x 8192 (tools/bench_bq.py), <RB, tile columns>: <1,128> 208.6 us, <2,64> 213.5 us, <2,128> 166.6 us
// (80.6 % of HBM), <4,64> 170.4 us.  The 128-row tile halves the LDS re-reads of the candidate fragments per byte of A; the
// 64-row tile is kept for short problems, where it gives twice as many workgroups.
// fp32, measured at 65536 x 8192: <1> 64-row tile 368-395 us, <2> 128-row tile 335.7 us (80 % of HBM), <4> 336.8 us.
struct BatchTile { int rows, f32_wg_per_cu, bf16_wg_per_cu; };
const BatchTile kBatchTiles[2] = {{64, 3, 2}, {128, 2, 1}};

// The grid of product 1 on `rows_total` rows: the tile variant (0: 64-row tile, 1: 128-row tile), the row groups per
// workgroup and the number of workgroups (rows of q_part).
struct BatchGrid { int variant; int64_t gpw, nwg; };
static BatchGrid batch_grid(const fos_problem* p, int64_t rows_total) {
  const bool is_bf16 = p->dtype == FOS_BF16;
  const int variant = rows_total >= 128 * (int64_t)p->ncu ? 1 : 0;
  const int rows = kBatchTiles[variant].rows;
  const int per_cu = is_bf16 ? kBatchTiles[variant].bf16_wg_per_cu : kBatchTiles[variant].f32_wg_per_cu;
  const int64_t ngroups = (rows_total + rows - 1) / rows;
  int64_t nwg = std::min<int64_t>(ngroups, per_cu * (int64_t)p->ncu);
  const int64_t gpw = (ngroups + nwg - 1) / nwg;
  nwg = (ngroups + gpw - 1) / gpw;
  return {variant, gpw, nwg};
}

// Product 1 (fos_internal.hpp BatchLaunch): the form follows from what the launch is given, and a form that is not in
// kBatchForms (a right-hand-side block with a fold mask, say) is refused before any launch; no entry point asks for one.
int launch_batch_product(fos_problem* p, const BatchLaunch& L, int* nwg_out) {
  const BatchForm want{L.rout != nullptr, L.bblock, L.fold_of_row ? (L.rout ? fos::FOLD_TRAIN : fos::FOLD_HELD) : fos::FOLD_OFF,
                       (L.use_b && p->loss == FOS_LOSS_LOGISTIC) ? fos::LOSS_LOGISTIC : fos::LOSS_SQUARED, L.row_weight != nullptr};
  const BatchEntry* hit = std::find_if(std::begin(kBatchForms), std::end(kBatchForms), [&](const BatchEntry& c) {
    return c.form.store == want.store && c.form.bblock == want.bblock && c.form.fold == want.fold && c.form.loss == want.loss &&
           c.form.weight == want.weight;
  });
  if (hit == std::end(kBatchForms)) return fail(FOS_ERR_STATE, "launch_batch_product: product 1 has no such form");
  const BatchEntry& e = *hit;
  const BatchGrid g = batch_grid(p, L.rows);
  const int use_b = (L.use_b && L.b) ? 1 : 0;
  const fos::FoldHeld held = L.held ? *L.held : fos::FoldHeld{};
  if (p->dtype == FOS_BF16)
    hipLaunchKernelGGL(e.bf16[g.variant], dim3((unsigned)g.nwg), dim3(fos::BT_THREADS), 0, p->stream, (const fos::bf16_t*)L.A,
                       p->lda, L.b, use_b, L.rows, (int)p->n, (const unsigned short*)p->cand.xp.get(), g.gpw, p->cand.q_part, L.rout,
                       L.stopped, L.fold_of_row, held, L.row_weight);
  else
    hipLaunchKernelGGL(e.f32[g.variant], dim3((unsigned)g.nwg), dim3(fos::BT_THREADS), 0, p->stream, (const float*)L.A, p->lda,
                       L.b, use_b, L.rows, (int)p->n, p->cand.xp, g.gpw, p->cand.q_part, L.rout, L.stopped, L.fold_of_row, held,
                       L.row_weight);
  LAUNCH_CHECK();
  *nwg_out = (int)g.nwg;
  return FOS_OK;
}

// need_squared's refusal of a problem with coordinate data: only the update of the two-product lockstep applies the factors
// and the bounds, so no other form may answer for such a problem.
int coord_refusal(const fos_problem* p, const char* fn) {
  if (p && has_coord(p))
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": not served on a problem with penalty factors or bounds (fos_coord_bind); "
                                     "with the squared or the logistic loss they run through fos_fista_run_multi / _run_multi_folds");
  return FOS_OK;
}

// ... and of a problem with feature groups: only the three update launches of the two-product lockstep apply the group prox.
int fgroup_refusal(const fos_problem* p, const char* fn) {
  if (p && has_fgroups(p))
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": not served on a problem with feature groups (fos_feature_groups_bind); "
                                     "with the squared or the logistic loss they run through fos_fista_run_multi / _run_multi_folds");
  return FOS_OK;
}

// ... and of a problem with the Huber or the squared-hinge loss: only the link kernel between the two products forms its residual.
int link_refusal(const fos_problem* p, const char* fn) {
  if (p && link_loss(p))
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": not served on a problem with the Huber or the squared-hinge loss "
                                     "(fos_problem_set_link_loss); like the logistic loss these run through fos_fista_run_multi / "
                                     "_run_multi_folds, fos_residual_batch / _folds and fos_gradient_batch");
  return FOS_OK;
}

int need_squared(const fos_problem* p, const char* fn) {
  if (p && p->row_weight != nullptr)
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": not served on a problem with row weights (fos_row_weights_bind); the "
                                     "weighted squared and logistic losses run through fos_fista_run_multi / _run_multi_folds and fos_residual_batch / "
                                     "_folds");
  if (int rc = link_refusal(p, fn)) return rc;
  if (p && p->loss != FOS_LOSS_SQUARED)
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + (p->loss == FOS_LOSS_MULTINOMIAL
                                                             ? ": not served on a multinomial problem (fos_problem_set_multinomial); the multinomial "
                                                             : ": not served on a logistic problem (fos_problem_set_loss); the logistic ") +
                                     "loss runs through fos_fista_run_multi / _run_multi_folds and fos_residual_batch / _folds");
  if (int rc = fgroup_refusal(p, fn)) return rc;
  return coord_refusal(p, fn);
}

bool fold_held_block(const int32_t* held, int nv, fos::FoldHeld* out) {
  for (int j = 0; j < fos::BT_NV; ++j) {
    const int32_t h = j < nv ? held[j] : -1;
    if (h < -1 || h > 254) return false;
    out->id[j] = (int8_t)h;                        // -1 is the byte 255, which no row carries
  }
  return true;
}

bool softmax_groups_ok(const fos_problem* p, int nv, const int32_t* held) {
  const int C = p->classes;
  if (C < 2 || nv % C != 0) return false;
  for (int j = 0; held && j < nv; ++j)
    if (held[j] != held[j / C * C]) return false;
  return true;
}

// The link kernel (softmax_link.hpp) behind product 1 on one row panel of a multinomial problem.  One thread per row: the
// panel has at most 256 * ncu rows, so the grid is at most ncu workgroups and q_part (3 * ncu + 8 rows) holds its partials.
int launch_softmax_link(fos_problem* p, int64_t row0, int64_t rows, int nv, int fold, const uint8_t* fold_of_row,
                        const fos::FoldHeld* held, double* q_part, int* nwg_out) {
  if (p->loss != FOS_LOSS_MULTINOMIAL || rows < 1 || rows > p->multi.panel_rows || !softmax_groups_ok(p, nv, nullptr) ||
      ((fold != fos::FOLD_OFF) && (!fold_of_row || !held)))
    return fail(FOS_ERR_STATE, "launch_softmax_link: not a panel of a multinomial problem");
  const int nwg = (int)std::min<int64_t>((rows + fos::SL_THREADS - 1) / fos::SL_THREADS, p->ncu);
  const fos::FoldHeld hb = held ? *held : fos::FoldHeld{};
  const float* w = p->row_weight ? p->row_weight + row0 : nullptr;
  const uint8_t* ids = fold != fos::FOLD_OFF ? fold_of_row + row0 : nullptr;
#define FOS_LINK(F, W)                                                                                                          \
  hipLaunchKernelGGL((fos::softmax_link_kernel<fos::F, W>), dim3(nwg), dim3(fos::SL_THREADS), 0, p->stream, p->multi.rbuf16.get(), \
                     rows, p->b + row0, p->classes, nv, w, ids, hb, q_part, (const int*)nullptr)
  if (fold == fos::FOLD_TRAIN) { if (w) FOS_LINK(FOLD_TRAIN, true); else FOS_LINK(FOLD_TRAIN, false); }
  else if (fold == fos::FOLD_HELD) { if (w) FOS_LINK(FOLD_HELD, true); else FOS_LINK(FOLD_HELD, false); }
  else { if (w) FOS_LINK(FOLD_OFF, true); else FOS_LINK(FOLD_OFF, false); }
#undef FOS_LINK
  LAUNCH_CHECK();
  *nwg_out = nwg;
  return FOS_OK;
}

// The link kernel (pointwise_link.hpp) behind product 1 on one row panel of a Huber or squared-hinge problem.  One lane per
// 16-byte quad of a row, grid-stride: at most 2 * ncu workgroups, within the 3 * ncu + 8 rows of cand.q_part.
int launch_pointwise_link(fos_problem* p, int64_t row0, int64_t rows, int nv, int fold, const uint8_t* fold_of_row,
                          const fos::FoldHeld* held, double* q_part, int* nwg_out) {
  if (!link_loss(p) || rows < 1 || rows > p->multi.panel_rows || nv < 1 || nv > fos::BT_NV ||
      ((fold != fos::FOLD_OFF) && (!fold_of_row || !held)))
    return fail(FOS_ERR_STATE, "launch_pointwise_link: not a panel of a Huber or squared-hinge problem");
  const int nwg = (int)std::min<int64_t>((4 * rows + fos::PL_THREADS - 1) / fos::PL_THREADS, 2 * (int64_t)p->ncu);
  const fos::FoldHeld hb = held ? *held : fos::FoldHeld{};
  const float* w = p->row_weight ? p->row_weight + row0 : nullptr;
  const uint8_t* ids = fold != fos::FOLD_OFF ? fold_of_row + row0 : nullptr;
  const float c = (float)p->link_param;
#define FOS_LINK(K, F, W)                                                                                                           \
  hipLaunchKernelGGL((fos::pointwise_link_kernel<fos::K, fos::F, W>), dim3(nwg), dim3(fos::PL_THREADS), 0, p->stream,              \
                     p->multi.rbuf16.get(), rows, p->b + row0, c, nv, w, ids, hb, q_part, (const int*)nullptr)
#define FOS_LINK_FORM(K)                                                                                              \
  if (fold == fos::FOLD_TRAIN) { if (w) FOS_LINK(K, FOLD_TRAIN, true); else FOS_LINK(K, FOLD_TRAIN, false); }         \
  else if (fold == fos::FOLD_HELD) { if (w) FOS_LINK(K, FOLD_HELD, true); else FOS_LINK(K, FOLD_HELD, false); }       \
  else { if (w) FOS_LINK(K, FOLD_OFF, true); else FOS_LINK(K, FOLD_OFF, false); }
  if (p->loss == FOS_LOSS_HUBER) { FOS_LINK_FORM(LINK_HUBER) } else { FOS_LINK_FORM(LINK_SQUARED_HINGE) }
#undef FOS_LINK_FORM
#undef FOS_LINK
  LAUNCH_CHECK();
  *nwg_out = nwg;
  return FOS_OK;
}

// q[j] = sum_i R[i][j]^2 of an m x 16 residual block (column-sharded candidate pass, after the sum over the ranks)
__global__ __launch_bounds__(256) void colnorms16_partials_kernel(const float* __restrict__ R, int64_t m, double* __restrict__ part,
                                                                 const int* stopped) {
  if (stopped != nullptr && *stopped != 0) return;
  __shared__ double ws[16][17];
  const int j = threadIdx.x & 15, sub = threadIdx.x >> 4;          // 16 rows per trip, a 64-byte row of R per 16 lanes
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 16 + sub; i < m; i += (int64_t)gridDim.x * 16) {
    const double v = (double)R[i * fos::BT_NV + j];
    acc += v * v;
  }
  ws[sub][j] = acc;
  __syncthreads();
  if (threadIdx.x < 16) {
    double t = 0.0;
    for (int s = 0; s < 16; ++s) t += ws[s][threadIdx.x];
    part[(int64_t)blockIdx.x * fos::BT_NV + threadIdx.x] = t;
  }
}
__global__ __launch_bounds__(256) void unsum16_if_stopped_kernel(float* __restrict__ v, int64_t count, float scale, const int* stopped) {
  if (*stopped == 0) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) v[i] *= scale;
}

// Product 1 without R on all rows of the problem (A, rows and rout of L are set here; the candidates are packed) ->
// out16[j] (device) = the sum of q_part[.][j], summed over the ranks of a row-sharded problem.
static int residual_batch_sums(fos_problem* p, BatchLaunch L, double* out16) {
  L.A = p->A; L.rows = p->m; L.rout = nullptr;
  int rc = prof_mark(p, true);
  if (rc) return rc;
  int nwg = 0;
  if ((rc = launch_batch_product(p, L, &nwg))) return rc;
  if ((rc = prof_mark(p, false))) return rc;
  hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, p->cand.q_part, nwg, fos::BT_NV, out16);
  LAUNCH_CHECK();
  return reduce_across(p, out16, fos::BT_NV, true);      // sharded: ||A dlt_j||^2 = sum over the row blocks
}

// q[j] = ||A Xp_j - use_b*b||^2 -> out16 (device); Xp already in p->cand.xp.
int launch_residual_batch(fos_problem* p, int use_b, double* out16, const int* stopped, const float* b16) {
  BatchLaunch L{};
  L.use_b = use_b; L.stopped = stopped;
  if (p->col_sharded) {
    int rc = prof_mark(p, true);
    if (rc) return rc;
    int nwg = 0;
    // Column-sharded: ||A dlt_j||^2 = ||sum_p A_p dlt_{j,p}||^2.  Every rank's product 1 keeps its partial residuals
    // (m x 16 floats), ONE all-reduce sums the blocks of all 16 candidates (4 MiB at m = 65536), the column norms follow.
    if ((rc = p->ws.rcols16.reserve((size_t)p->m * fos::BT_NV))) return rc;
    L.A = p->A; L.b = p->comm->rank == 0 ? p->b : nullptr; L.rows = p->m; L.rout = p->ws.rcols16;
    if ((rc = launch_batch_product(p, L, &nwg))) return rc;
    if ((rc = prof_mark(p, false))) return rc;
    if (stopped != nullptr) {        // a no-op product leaves the last SUM in place: divide it back before the in-place all-reduce
      hipLaunchKernelGGL(unsum16_if_stopped_kernel, dim3(grid_1d(p->m * fos::BT_NV, 256, 1024)), dim3(256), 0, p->stream,
                         p->ws.rcols16, p->m * fos::BT_NV, 1.0f / (float)p->comm->nranks, stopped);
      LAUNCH_CHECK();
    }
    if ((rc = reduce_across(p, p->ws.rcols16, (size_t)p->m * fos::BT_NV, false))) return rc;
    const int g = grid_1d(p->m, 16 * 16, 3 * p->ncu);
    hipLaunchKernelGGL(colnorms16_partials_kernel, dim3(g), dim3(256), 0, p->stream, p->ws.rcols16, p->m, p->cand.q_part, stopped);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, p->cand.q_part, g, fos::BT_NV, out16);
    LAUNCH_CHECK();
    return FOS_OK;
  }
  L.b = b16 ? b16 : p->b; L.bblock = b16 != nullptr;
  return residual_batch_sums(p, L, out16);
}

// ---- multi-lambda lockstep run ----------------------------------------------------------------------------------

// BBLOCK: b is the m x 16 right-hand-side block (one b per vector)
template <int THREADS, int K, int NVEC, bool BBLOCK = false>
void multi_launch(const float* A, int64_t lda, const float* b, int64_t m, int n, fos::MultiY ys, int64_t rpw,
                         float* slabs, double* rr_part, int nwg, hipStream_t st) {
  hipLaunchKernelGGL((fos::gemv_multi_kernel<float, THREADS, K, 2, NVEC, 2, BBLOCK>), dim3(nwg), dim3(THREADS), 0, st, A, lda,
                     b, m, n, ys, rpw, slabs, rr_part);
}
MultiLaunch find_multi(int64_t n, int nv, bool bblock) {
  static const MultiLaunch small[3] = {multi_launch<256, 4, 2>, multi_launch<256, 4, 3>, multi_launch<256, 4, 4>};
  static const MultiLaunch big[3] = {multi_launch<512, 4, 2>, multi_launch<512, 4, 3>, multi_launch<512, 4, 4>};
  static const MultiLaunch small_rhs[3] = {multi_launch<256, 4, 2, true>, multi_launch<256, 4, 3, true>,
                                           multi_launch<256, 4, 4, true>};
  static const MultiLaunch big_rhs[3] = {multi_launch<512, 4, 2, true>, multi_launch<512, 4, 3, true>,
                                         multi_launch<512, 4, 4, true>};
  if (nv < 2 || nv > 4) return nullptr;
  if (n <= 4096) return (bblock ? small_rhs : small)[nv - 2];
  if (n <= 8192) return (bblock ? big_rhs : big)[nv - 2];
  return nullptr;
}

int stage_b16(fos_problem* p, const float* B, int64_t ldb, int nv) {
  if (int rc = p->ws.b16.reserve((size_t)p->m * fos::BT_NV)) return rc;
  hipLaunchKernelGGL(fos::stage_b16_kernel, dim3(grid_1d(p->m * fos::BT_NV, 256, 4 * p->ncu)), dim3(256), 0, p->stream, B,
                     ldb, nv, p->m, p->ws.b16);
  LAUNCH_CHECK();
  return FOS_OK;
}

// The matrix-core passes (16 candidates / 16 weights) need the aligned layout only - not a streaming plan: rows of 65..128
// columns run the chunk-per-lane pass (p->pass.tall) and keep them; n <= 64 may be ragged / misaligned and does not.
bool batch_supported(const fos_problem* p) { return p->pass.path == 0 && (!p->pass.tall || p->n > fos::TL_MAX_N); }   // fp32: f32 MFMA; bf16: 3-term bf16 MFMA

// ---- fp64 multi-point pass on the matrix cores (gram_batch_dd.hpp) ---------------------------------------------------
// The shapes of the fp32 matrix-core pair (run_multi_mfma): the aligned layout, fp32 and bf16, up to 16384 columns, any
// number of row panels; not the two-pass / LDS-resident / n <= 64 plans, column blocks, the y-in-LDS rows or sharding.
bool pair_dd_multi_supported(const fos_problem* p) {
  return batch_supported(p) && !p->pass.colblock && !p->pass.resident && !p->col_sharded && !p->comm && p->pass.entry != wide_entry(p->dtype) &&
         p->n <= 16384;
}

// Geometry and workspace, decided on first use.  Panel and row splits of product 2 as in run_multi_mfma; product 1 gives a
// workgroup groups of 64 rows, at most two workgroups per CU (51 KiB of LDS each for fp32).
constexpr int DM_P1_PER_CU = 2;
int ensure_dd_multi(fos_problem* p) {
  if (p->dm.planned) return FOS_OK;
  const int64_t n = p->n;
  p->dm.n_pad = (n + fos::DM_COLS - 1) / fos::DM_COLS * fos::DM_COLS;
  p->dm.panel_rows = std::min<int64_t>(256 * (int64_t)p->ncu, (p->m + 255) / 256 * 256);
  const int64_t strips = (n + fos::DM_COLS - 1) / fos::DM_COLS;
  int64_t splits = std::max<int64_t>(1, (2 * (int64_t)p->ncu + strips - 1) / strips);
  splits = std::min<int64_t>(splits, std::max<int64_t>(1, p->dm.panel_rows / 256));
  p->dm.rows_per_split = ((p->dm.panel_rows + splits - 1) / splits + fos::DM_ROWS - 1) / fos::DM_ROWS * fos::DM_ROWS;
  p->dm.splits = (int)((p->dm.panel_rows + p->dm.rows_per_split - 1) / p->dm.rows_per_split);
  const int64_t panels = (p->m + p->dm.panel_rows - 1) / p->dm.panel_rows;
  int rc;
  if ((rc = p->dm.xd.reserve((size_t)p->dm.n_pad * fos::BT_NV)) || (rc = p->dm.rdd.reserve((size_t)p->dm.panel_rows * fos::BT_NV)) ||
      (rc = p->dm.slabs.reserve((size_t)p->dm.splits * fos::BT_NV * n)) ||
      (rc = p->dm.q_part.reserve((size_t)panels * DM_P1_PER_CU * p->ncu * fos::BT_NV)))
    return rc;
  p->dm.planned = true;
  return FOS_OK;
}

// Per panel: product 1 (R = A_panel X - B16_panel and its squared column norms), product 2 (slabs (+)= R^T A_panel), each
// bracketed by the launch profiler; then one launch sums the slab sets into the gradients and folds ||r||^2.
template <typename T>
int run_pair_dd_multi(fos_problem* p, const fos::DdMultiCols& c, int ncols, unsigned live, double alpha2, const float* b16) {
  const int64_t n = p->n, esz = sizeof(T);
  hipLaunchKernelGGL(fos::xd_pack_kernel, dim3(grid_1d(p->dm.n_pad * fos::BT_NV, 256, 4 * p->ncu)), dim3(256), 0, p->stream, c,
                     live, (int)n, (int)p->dm.n_pad, p->dm.xd);
  LAUNCH_CHECK();
  const int64_t strips = (n + fos::DM_COLS - 1) / fos::DM_COLS;
  int64_t nparts = 0;
  int rc;
  for (int64_t row0 = 0, panel = 0; row0 < p->m; row0 += p->dm.panel_rows, ++panel) {
    const int64_t rows = std::min<int64_t>(p->dm.panel_rows, p->m - row0);
    const T* Ap = reinterpret_cast<const T*>(reinterpret_cast<const char*>(p->A) + (size_t)row0 * p->lda * esz);
    const int64_t ngroups = (rows + fos::DM_ROWS - 1) / fos::DM_ROWS;
    int64_t nwg = std::min<int64_t>(ngroups, DM_P1_PER_CU * (int64_t)p->ncu);
    const int64_t gpw = (ngroups + nwg - 1) / nwg;
    nwg = (ngroups + gpw - 1) / gpw;
    if ((rc = prof_mark(p, true))) return rc;
    hipLaunchKernelGGL(fos::residual_dd_mfma_kernel<T>, dim3((unsigned)nwg), dim3(fos::DM_THREADS), 0, p->stream, Ap, p->lda,
                       b16 + row0 * fos::BT_NV, rows, (int)n, (const double*)p->dm.xd, gpw, p->dm.q_part + nparts * fos::BT_NV,
                       p->dm.rdd);
    LAUNCH_CHECK();
    if ((rc = prof_mark(p, false))) return rc;
    nparts += nwg;
    const dim3 grid((unsigned)strips, (unsigned)p->dm.splits);
    if ((rc = prof_mark(p, true))) return rc;
    if (panel)
      hipLaunchKernelGGL((fos::gram_dd_mfma_kernel<T, true>), grid, dim3(fos::DM_THREADS), 0, p->stream, Ap, p->lda, rows,
                         (int)n, (const double*)p->dm.rdd, p->dm.rows_per_split, p->dm.slabs, n);
    else
      hipLaunchKernelGGL((fos::gram_dd_mfma_kernel<T, false>), grid, dim3(fos::DM_THREADS), 0, p->stream, Ap, p->lda, rows,
                         (int)n, (const double*)p->dm.rdd, p->dm.rows_per_split, p->dm.slabs, n);
    LAUNCH_CHECK();
    if ((rc = prof_mark(p, false))) return rc;
  }
  hipLaunchKernelGGL(fos::pair_dd_multi_finish_kernel, dim3(grid_1d(n, 256, 64), ncols), dim3(256), 0, p->stream,
                     (const double*)p->dm.slabs, p->dm.splits, (int)n, (const double*)p->dm.q_part, (int)nparts, alpha2, c);
  LAUNCH_CHECK();
  return FOS_OK;
}

// The dispatch of the fp64 multi-point pass: one entry per storage type (a table of its own, apart from the streaming menus)
typedef int (*PairDdMultiRun)(fos_problem*, const fos::DdMultiCols&, int, unsigned, double, const float*);
struct PairDdMultiEntry { int dtype; PairDdMultiRun run; };
const PairDdMultiEntry kPairDdMulti[] = {
    {FOS_F32, run_pair_dd_multi<float>},
    {FOS_BF16, run_pair_dd_multi<fos::bf16_t>},
};

int pair_dd_multi(fos_problem* p, const fos::DdMultiCols& c, int ncols, unsigned live, double alpha2, const float* b16) {
  if (!pair_dd_multi_supported(p))
    return fail(FOS_ERR_UNSUPPORTED, "fos_gemv_pair_dd_multi: no matrix-core pair for this shape (needs the aligned streaming "
                                     "layout, 65..16384 columns, unsharded)");
  if (ncols < 1) return FOS_OK;
  int rc = ensure_dd_multi(p);
  if (rc) return rc;
  for (const auto& e : kPairDdMulti)
    if (e.dtype == p->dtype) return e.run(p, c, ncols, live, alpha2, b16);
  return fail(FOS_ERR_UNSUPPORTED, "fos_gemv_pair_dd_multi: storage type not served");
}

// A caller vector the fused prologue can read with 16-byte loads.
int aligned_vec(fos_problem* p, const float* v, const float** out) {
  if ((reinterpret_cast<uintptr_t>(v) & 15u) == 0) {
    *out = v;
    return FOS_OK;
  }
  HIP_TRY(hipMemcpyAsync(p->ws.ybuf, v, (size_t)p->n * sizeof(float), hipMemcpyDeviceToDevice, p->stream));
  *out = p->ws.ybuf;
  return FOS_OK;
}

// Row order of the streaming pass.  Contiguous blocks per workgroup keep 256 streams 8-256 MiB apart; dealing the rows
// round-robin (IL) makes all CUs read ONE contiguous window (256 rows = 16 MiB at 64 KiB rows) that sweeps the matrix.
// profiles/r03_row_order.md (tools/skew_bench, tools/order_probe.py, in-bench A/B): on a quiet device the two are within
// 2 % of each other either way (8 GiB: blocks 1186 us / IL 1208 us; 16 GiB: 2425-2458 / 2394-2417; 32 GiB: 4800-4840 /
// 4777-4823; 64 GiB: 9546 / 9525), but for seconds after ANY large free on the device (this process's or the previous
// one's - the driver releases and clears VRAM in the background) the block form loses 3-6 % while the interleaved form
// does not move: cfg4 in bench.py, three fresh processes each: blocks 9989-9996 us, interleaved 9550-9571 us.  From 12 GiB
// on the interleaved form is never behind, so it is the default there; below, blocks keep their quiet-state edge.
bool il_default(const fos_problem* p) {
  const int64_t bytes = p->m * p->n * (p->dtype == FOS_F32 ? 4 : 2);
  return bytes >= (12ll << 30);
}

// the streaming kernels' layout: whole 16-byte chunks per row, rows and the matrix 16-byte aligned
bool vec_layout(const fos_problem* p) {
  const int epc = epc_of(p->dtype);
  return (p->n % epc == 0) && (p->lda % epc == 0) && ((reinterpret_cast<uintptr_t>(p->A) & 15u) == 0);
}
// the one-workgroup resident loop has no exchange step
void plan_resident(fos_problem* p) { p->pass.resident = fos::resident_fits(p->m, p->n) && p->allow_resident && p->comm == nullptr; }
// The two-phase column-block plan: blocks of equal width (a multiple of 64 columns, at most the widest streaming geometry).
// Null where no streaming geometry with a column-block form covers that width.
const MenuEntry* colblock_entry(const fos_problem* p, int64_t* width) {
  const int64_t cap = 16384, blocks = (p->n + cap - 1) / cap;
  *width = ((p->n + blocks - 1) / blocks + 63) / 64 * 64;
  const MenuEntry* ce = default_entry(p->dtype, *width);
  return ce && ce->with_g_cb && ce->resid_only_cb ? ce : nullptr;
}
void plan_colblock(fos_problem* p, const MenuEntry* ce, int64_t width) {
  plan_fused(p, ce, 0);
  p->pass.colblock = true;
  p->pass.cb_width = width;
}

// Choose the kernel family for this problem (a fresh PassPlan); `flags` (FOS_PLAN_*) switch individual families off
// (fos_problem_replan).
void apply_plan(fos_problem* p, unsigned flags) {
  const int64_t n = p->n;
  p->plan_flags = flags;
  p->pass.vec4 = (n % 4 == 0);
  p->allow_resident = !(flags & FOS_PLAN_NO_RESIDENT);
  p->il = (flags & FOS_PLAN_INTERLEAVE) ? true : (flags & FOS_PLAN_NO_INTERLEAVE) ? false : il_default(p);
  plan_resident(p);
  const bool vec_ok = vec_layout(p);
  int64_t cb_width = 0;
  const MenuEntry* e = vec_ok ? default_entry(p->dtype, n) : nullptr;
  if ((n <= fos::TL_MAX_N || (n <= tlr_max_n(p->dtype) && vec_ok)) && !(flags & FOS_PLAN_NO_TALL))
    plan_tall(p, tall_entry(p->dtype, n, p->lda, p->A));
  else if (e) plan_fused(p, e, 0);
  else if (vec_ok && n <= fos::WD_MAX_N && !(flags & FOS_PLAN_NO_WIDE)) plan_fused(p, wide_entry(p->dtype), 0);
  else if (const MenuEntry* ce = (vec_ok && !(flags & FOS_PLAN_NO_COLBLOCK)) ? colblock_entry(p, &cb_width) : nullptr)
    plan_colblock(p, ce, cb_width);
  else plan_fallback(p);
}

int invalidate(fos_problem* p, unsigned changed) {
  // these two follow launches of the same call or tuning loop: the stream drains before their buffers go
  if (changed & (IN_TUNE_DD | IN_CLUSTER)) HIP_TRY(hipStreamSynchronize(p->stream));
  if (changed & IN_PLAN) p->pass.reset();
  if (changed & (IN_PLAN | IN_TUNE | IN_COMM)) p->pk.reset();         // a tuned grid or row order keeps serving: the next run packs again
  if (changed & IN_COMM) plan_resident(p);
  if (changed & (IN_PLAN | IN_TUNE | IN_TUNE_DD | IN_COMM)) p->dd.reset();
  if (changed & (IN_PLAN | IN_COMM | IN_CLUSTER)) p->multi.reset();
  return FOS_OK;
}

// Up to 16 state machines in lockstep on the matrix cores (run_multi_mfma).
// One-read form (cluster_pass.hpp): fp32, 2049..16384 columns in strips of 1024 -> 4, 8 or 16 members per cluster, all CUs
// busy, at least 8 panels per cluster; FOS_PLAN_CLUSTER / FOS_PLAN_NO_CLUSTER force it on (where served) / off.
// Planner default (profiles/r03_cluster_crossover.md, 16 weights, us per iteration, two products -> one read): the one-read
// form wins where every member of a cluster has a full 1024-column strip and the matrix is large - 131072 x 4096 826 -> 640,
// 524288 x 4096 3306 -> 2407, 65536 x 8192 670 -> 643, 262144 x 8192 2668 -> 2430 - ties at 32768 x 8192 and loses with
// idle members (6144 columns +10 %, 3072 +5 %) and at 16 members (131072 x 16384 +5 %).
int plan_multi_mfma(fos_problem* p) {
  if (p->multi.planned) return FOS_OK;
  int rc;
  const bool is_bf16 = p->dtype == FOS_BF16;
  const int cs_need = (int)((p->n + fos::CP_W - 1) / fos::CP_W);
  const bool cluster_wins = (p->n == 4096 || p->n == 8192) && p->m * p->n >= (1ll << 29) && !p->comm;
  const bool want_cluster = p->cp_mode == 1 || (p->cp_mode == 0 && cluster_wins);
  if (want_cluster && !is_bf16 && p->ncu % 8 == 0) {
    const int cs = cs_need <= 2 ? 0 : cs_need <= 4 ? 4 : cs_need <= 8 ? 8 : cs_need <= 16 ? 16 : 0;
    if (cs && (p->ncu / 8) % cs == 0 && p->m >= (int64_t)(p->ncu / cs) * fos::CP_ROWS * 8) {
      p->multi.cp_cs = cs;
      p->multi.cp_clusters = p->ncu / cs;
      p->multi.cp_rows_per_cluster = ((p->m + p->multi.cp_clusters - 1) / p->multi.cp_clusters + fos::CP_ROWS - 1) / fos::CP_ROWS * fos::CP_ROWS;
      if ((rc = p->multi.cp_xchg.reserve((size_t)p->ncu * fos::CP_SLOTS * 256)) ||
          (rc = p->multi.cp_flags.reserve((size_t)p->ncu * fos::CP_FLAG_STRIDE)) || (rc = p->multi.cp_error.reserve(1)))
        return rc;
      HIP_TRY(hipMemsetAsync(p->multi.cp_flags, 0, (size_t)p->ncu * fos::CP_FLAG_STRIDE * sizeof(unsigned), p->stream));
      HIP_TRY(hipMemsetAsync(p->multi.cp_error, 0, sizeof(int), p->stream));
    }
  }
  // Panel: product 1 gives a workgroup 64-128 whole rows, so it needs >= 128 * CUs * 2 rows to fill the chip; row splits of
  // product 2: enough (strip, split) workgroups for two per CU.  (A panel that fits the Infinity Cache - ~3000 rows at
  // n = 8192 - would need a split-K product 1; see DESIGN.md "Multi-lambda".)
  const int64_t rows = 256 * (int64_t)p->ncu;
  p->multi.panel_rows = std::min<int64_t>(rows, (p->m + 255) / 256 * 256);
  if (p->col_sharded && p->comm->kind != 0) {          // mesh transport: a panel's 16 residual columns are one message
    const int64_t fit = (int64_t)(p->comm->cap_bytes / (fos::BT_NV * sizeof(float))) / 256 * 256;
    if (fit < 256) return fail(FOS_ERR_ARG, "fos_fista_run_multi: the communicator's inbox rows hold less than one 256-row "
                                            "panel of 16 residual columns (16 KiB)");
    p->multi.panel_rows = std::min<int64_t>(p->multi.panel_rows, fit);
  }
  const int64_t strips = (p->n + (is_bf16 ? fos::GQ_COLS : fos::GB_COLS) - 1) / (is_bf16 ? fos::GQ_COLS : fos::GB_COLS);
  int64_t splits = std::max<int64_t>(1, (2 * (int64_t)p->ncu + strips - 1) / strips);
  splits = std::min<int64_t>(splits, std::max<int64_t>(1, p->multi.panel_rows / 256));
  p->multi.gram_rows_per_split = ((p->multi.panel_rows + splits - 1) / splits + fos::GB_ROWS - 1) / fos::GB_ROWS * fos::GB_ROWS;
  p->multi.gram_splits = (int)((p->multi.panel_rows + p->multi.gram_rows_per_split - 1) / p->multi.gram_rows_per_split);
  if (p->multi.cp_cs) p->multi.gram_splits = p->multi.cp_clusters;      // one slab set per cluster
  if ((rc = p->multi.rbuf16.reserve((size_t)p->multi.panel_rows * fos::BT_NV)) ||
      (rc = p->multi.slabs16.reserve((size_t)p->multi.gram_splits * fos::BT_NV * p->n)))
    return rc;
  p->multi.planned = true;
  return FOS_OK;
}

// ---- fp64-accumulating pass (L-BFGS fg) -----------------------------------------------------------------------------
// Geometry and workspace of fos_gemv_pair_dd, decided on first use: the tall kernels and the resident kernel serve it as
// they are (they accumulate in fp64 anyway), streaming shapes get the ACC = double instantiation of gemv_pair_kernel,
// everything else (ragged / misaligned layouts, rows wider than the dd menu) the fp64 two-pass kernels.
int ensure_dd(fos_problem* p) {
  if (p->dd.planned || p->pass.resident) return FOS_OK;
  int rc;
  int nslabs = 0;
  int64_t stride = p->n;
  int n_rr = 0;
  if (p->pass.tall) {
    nslabs = p->pass.nwg; stride = p->pass.slab_stride; n_rr = p->pass.nwg;
  } else {
    const DdEntry* e = nullptr;
    if (p->pass.path == 0 && !p->col_sharded)      // column-sharded: the two-pass form, r all-reduced between the passes
      for (const auto& c : kDdMenu)
        if (c.dtype == p->dtype && (int64_t)c.threads * c.k * epc_of(p->dtype) >= p->n) { e = &c; break; }
    if (e) {
      p->dd.entry = e;
      // fp64 form: two workgroups per CU for the 256-thread geometries (they hold 2 waves per SIMD at most 256 VGPRs
      // each); four for the one-chunk geometry (76 VGPRs; 1048576 x 1024: 723 -> 660 us = 81 % of 8 TB/s, tools/dd_bench;
      // the two-chunk geometry is best at two: 524288 x 2048 87.5 % against 82 %)
      // Swept on the whole fg (pass + fp64 slab sum, tools/wg_sweep_dd.py, profiles/r03_wg_sweep.txt): the single-wave
      // geometries want eight per CU (2097152 x 256: 378 -> 348 us, 1677568 x 320: 420 -> 357 us) except full two-chunk rows
      // (1048576 x 512: four, 308 us against 336); two-chunk 256-thread rows that leave 30 % of the lanes without a chunk four
      // instead of two (419328 x 1280: 403 -> 371 us).
      const int64_t cap = (int64_t)e->threads * e->k * epc_of(p->dtype);
      const bool full = p->n * 10 > 9 * cap, sparse = p->n * 10 <= 7 * cap;
      int nwg = p->ncu * (e->threads >= 512 ? 1
                          : e->threads == 256 ? (e->k == 1 ? 4 : (e->k == 2 && sparse ? 4 : 2))
                                              : (e->k >= 3 || (e->k == 2 && full) ? 4 : 8));      // (64 x 3, 838656 x 640: 313 us at four, 331 at eight)
      const int64_t row_bytes = p->n * (p->dtype == FOS_F32 ? 4 : 2);
      // (below half a GiB the slab sum outweighs it: 200000 x 256 51 us with four per CU, 57 us with eight)
      if (e->threads == 64 && p->m * row_bytes < (512ll << 20)) nwg = std::min(nwg, 4 * p->ncu);
      const int64_t min_rows = std::max<int64_t>(2 * (int64_t)e->r, (65536 + row_bytes - 1) / row_bytes);   // fp64 slabs
      if (p->dd_nwg_hint > 0) nwg = p->dd_nwg_hint;
      if (p->m < (int64_t)nwg * min_rows) nwg = (int)std::max<int64_t>(1, p->m / min_rows);
      p->dd.rows_per_wg = (p->m + nwg - 1) / nwg;
      p->dd.nwg = (int)((p->m + p->dd.rows_per_wg - 1) / p->dd.rows_per_wg);
      nslabs = p->dd.nwg; n_rr = p->dd.nwg;
    } else {
      const int chunks = (int)std::max<int64_t>(1, std::min<int64_t>(64, p->m / 64));
      p->dd.rows_per_wg = (p->m + chunks - 1) / chunks;
      p->dd.two_pass_chunks = (int)((p->m + p->dd.rows_per_wg - 1) / p->dd.rows_per_wg);
      p->dd.nwg = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (p->m + 3) / 4));      // pass-1 grid
      nslabs = p->dd.two_pass_chunks; n_rr = p->dd.nwg;
      if ((rc = p->pass.rvec.reserve(p->m))) return rc;
    }
  }
  if ((rc = p->dd.rr.reserve(std::max(n_rr, 1))) || (rc = p->dd.slabs.reserve((size_t)nslabs * stride))) return rc;
  p->dd.planned = true;
  return FOS_OK;
}

// One launch of the one-read multi-lambda pass (cluster_pass.hpp): all members of a cluster must be resident (they are:
// one workgroup per CU).
template <int CS>
int launch_cluster_pass_cs(fos_problem* p) {
  auto kern = fos::cluster_pass_kernel<CS>;
  static std::atomic<uint64_t> done{0};
  if (raise_dynamic_lds(kern, fos::CP_LDS_BYTES, done)) return fail(FOS_ERR_HIP, "cluster pass: dynamic LDS size refused");
  const float* A = (const float*)p->A;
  int64_t lda = p->lda, m = p->m, rpc = p->multi.cp_rows_per_cluster, n_stride = p->n;
  int n = (int)p->n, n_pad = (int)p->cand.n_pad, xcd_aware = 1;
  const float* b = p->b;
  const float* xp = p->cand.xp;
  unsigned epoch = p->cp_epoch;
  // A PLAIN launch: #CUs workgroups with > 80 KiB of LDS each are co-resident by grid size - all a cooperative launch
  // would check (MI355X_MICROARCH.md "coop-launch") - every wait in the kernel is bounded, and a process that used
  // hipLaunchCooperativeKernel dies in rocprofv3's exit handler (tools/exit_probe.py, round 3).
  hipLaunchKernelGGL(kern, dim3((unsigned)(p->multi.cp_clusters * CS)), dim3(fos::CP_THREADS), (unsigned)fos::CP_LDS_BYTES, p->stream, A,
                     lda, b, m, n, n_pad, xp, rpc, xcd_aware, p->multi.cp_xchg, p->multi.cp_flags, epoch, p->multi.slabs16, n_stride, p->multi.cp_error);
  LAUNCH_CHECK();
  p->cp_epoch += (unsigned)(rpc / fos::CP_ROWS) + 16u;
  return FOS_OK;
}
int launch_cluster_pass(fos_problem* p) {
  switch (p->multi.cp_cs) {
    case 4: return launch_cluster_pass_cs<4>(p);
    case 8: return launch_cluster_pass_cs<8>(p);
    case 16: return launch_cluster_pass_cs<16>(p);
  }
  return fail(FOS_ERR_STATE, "cluster pass: no plan");
}


// Read-only streaming probe: what this box's HBM delivers to a kernel that does nothing but load (the context figure SURVEY.md
// 8d asks for beside the nominal 8 TB/s).  The fastest of 18 x 4 loads-only variants (tools/read_probe_sweep.hip,
// profiles/r03_read_probe_sweep.txt: 7.19 TB/s; grid-stride order 7.1, temporal loads 6.2, 4 workgroups per CU 6.1): one
// 512-thread workgroup per CU streams its own contiguous range with 8 independent 16-byte non-temporal loads in flight per
// thread - the access pattern of the single-pass kernel without its arithmetic.
// ORDER 0: every workgroup streams its own contiguous range; 1: all workgroups sweep one window, 8 KiB per workgroup and trip;
// 2: the same with 64 KiB per workgroup and trip - the interleaved row order of the product kernel at 64 KiB rows
template <int ORDER>
__global__ __launch_bounds__(512) void stream_read_kernel(const fos::f32x4* __restrict__ src, size_t n16, float* __restrict__ sink) {
  constexpr int UNR = 8, THREADS = 512;
  constexpr bool BLOCKS = ORDER == 0;
  fos::f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if constexpr (ORDER == 2) {
    constexpr size_t CH = (size_t)UNR * THREADS;       // 16-byte units per workgroup and trip = 64 KiB
    size_t base = (size_t)blockIdx.x * CH;
    for (; base + CH <= n16; base += (size_t)gridDim.x * CH) {
      fos::f32x4 v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) v[u] = __builtin_nontemporal_load(src + base + threadIdx.x + (size_t)u * THREADS);
#pragma unroll
      for (int u = 0; u < UNR; ++u) acc += v[u];
    }
    for (size_t i = base + threadIdx.x; i < n16 && i < base + CH; i += THREADS) acc += __builtin_nontemporal_load(src + i);
  } else if constexpr (BLOCKS) {                        // every workgroup streams its own contiguous range
    const size_t per = ((n16 + gridDim.x - 1) / gridDim.x + THREADS * UNR - 1) / (THREADS * UNR) * (THREADS * UNR);
    const size_t lo = per * blockIdx.x, hi = lo + per < n16 ? lo + per : n16;
    size_t i = lo + threadIdx.x;
    for (; i + (size_t)(UNR - 1) * THREADS < hi; i += (size_t)UNR * THREADS) {
      fos::f32x4 v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) v[u] = __builtin_nontemporal_load(src + i + (size_t)u * THREADS);
#pragma unroll
      for (int u = 0; u < UNR; ++u) acc += v[u];
    }
    for (; i < hi; i += THREADS) acc += __builtin_nontemporal_load(src + i);
  } else {                                              // all workgroups sweep one window (the interleaved row order's pattern)
    const size_t stride = (size_t)gridDim.x * THREADS;
    size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    for (; i + (UNR - 1) * stride < n16; i += UNR * stride) {
      fos::f32x4 v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) v[u] = __builtin_nontemporal_load(src + i + u * stride);
#pragma unroll
      for (int u = 0; u < UNR; ++u) acc += v[u];
    }
    for (; i < n16; i += stride) acc += __builtin_nontemporal_load(src + i);
  }
  const float t = fos::wave_sum((acc.x + acc.y) + (acc.z + acc.w));
  if ((threadIdx.x & 63) == 0) sink[blockIdx.x * 8 + (threadIdx.x >> 6)] = t;
}

}  // namespace fosapi

using namespace fosapi;

extern "C" {

const char* fos_last_error(void) { return g_err.c_str(); }
int fos_abi_version(void) { return FOS_ABI_VERSION; }

int fos_problem_create(fos_problem** out, const void* A, int64_t m, int64_t n, int64_t lda, int a_dtype,
                       const float* b, void* stream) {
  if (!out || !A || m <= 0 || n <= 0 || lda < n) return fail(FOS_ERR_ARG, "fos_problem_create: bad shape/pointer");
  if (a_dtype != FOS_F32 && a_dtype != FOS_BF16) return fail(FOS_ERR_ARG, "fos_problem_create: bad a_dtype");
  if (n > (int64_t)1 << 30) return fail(FOS_ERR_ARG, "fos_problem_create: n too large");
  fos_problem* p = new fos_problem();
  p->A = A; p->b = b; p->m = m; p->n = n; p->lda = lda; p->dtype = a_dtype;
  p->stream = reinterpret_cast<hipStream_t>(stream);
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
    delete p;
    return fail(FOS_ERR_HIP, "fos_problem_create: no HIP device");
  }
  p->ncu = prop.multiProcessorCount;
  apply_plan(p, 0);
  int rc;
  if ((rc = ensure_workspace(p)) || (rc = p->ws.gbuf_own.reserve(n + 4)) || (rc = p->ws.ybuf.reserve(n)) ||
      (rc = p->ws.dscal.reserve(256)) || (rc = p->ws.part.reserve(std::max<size_t>(1024, (n + fos::RCOLS - 1) / fos::RCOLS) * 4))) {
    delete p;
    return rc;
  }
  p->gbuf = p->ws.gbuf_own;
  *out = p;
  return FOS_OK;
}

int fos_problem_set_loss(fos_problem* p, int loss) {
  if (!p) return fail(FOS_ERR_ARG, "fos_problem_set_loss: null");
  if (loss != FOS_LOSS_SQUARED && loss != FOS_LOSS_LOGISTIC)
    return fail(FOS_ERR_ARG, "fos_problem_set_loss: unknown loss (the multinomial loss is set with fos_problem_set_multinomial)");
  if (loss == FOS_LOSS_LOGISTIC) {
    if (!p->b) return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_loss: a logistic problem needs b (the labels)");
    if (p->comm || p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_loss: sharded problems are not served");
    if (!pair_dd_multi_supported(p))
      return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_loss: the logistic loss runs on the matrix-core pair (aligned streaming "
                                       "layout, 65..16384 columns)");
  }
  p->loss = loss;                    // no buffer depends on the loss: nothing to invalidate
  p->link_param = 0.0;
  return FOS_OK;
}

int fos_problem_set_link_loss(int loss, double param, fos_problem* p) {
  if (!p) return fail(FOS_ERR_ARG, "fos_problem_set_link_loss: null problem");
  if (loss != FOS_LOSS_HUBER && loss != FOS_LOSS_SQUARED_HINGE)
    return fail(FOS_ERR_ARG, "fos_problem_set_link_loss: the loss is FOS_LOSS_HUBER or FOS_LOSS_SQUARED_HINGE");
  if (loss == FOS_LOSS_HUBER && !(std::isfinite(param) && param > 0.0))
    return fail(FOS_ERR_ARG, "fos_problem_set_link_loss: the Huber threshold is not finite and > 0");
  if (loss == FOS_LOSS_SQUARED_HINGE && param != 0.0)
    return fail(FOS_ERR_ARG, "fos_problem_set_link_loss: the squared hinge takes no parameter (param = 0)");
  if (!p->b) return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_link_loss: the Huber and squared-hinge losses need b");
  if (p->comm || p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_link_loss: sharded problems are not served");
  if (!pair_dd_multi_supported(p))
    return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_link_loss: the Huber and squared-hinge losses run on the matrix-core pair "
                                     "(aligned streaming layout, 65..16384 columns)");
  p->loss = loss;                    // no buffer depends on the loss or on its parameter: nothing to invalidate
  p->link_param = loss == FOS_LOSS_HUBER ? param : 0.0;
  return FOS_OK;
}

int fos_problem_get_link_loss(int* loss, double* param, const fos_problem* p) {
  if (!p || !loss || !param) return fail(FOS_ERR_ARG, "fos_problem_get_link_loss: null");
  *loss = link_loss(p) ? p->loss : 0;
  *param = link_loss(p) ? p->link_param : 0.0;
  return FOS_OK;
}

int fos_problem_set_multinomial(int classes, fos_problem* p) {
  if (!p) return fail(FOS_ERR_ARG, "fos_problem_set_multinomial: null problem");
  if (classes < 2 || classes > fos::BT_NV) return fail(FOS_ERR_ARG, "fos_problem_set_multinomial: classes outside 2..16");
  if (!p->b) return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_multinomial: a multinomial problem needs b (the class of every row)");
  if (p->comm || p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_multinomial: sharded problems are not served");
  if (!pair_dd_multi_supported(p))
    return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_multinomial: the multinomial loss runs on the matrix-core pair (aligned "
                                     "streaming layout, 65..16384 columns)");
  if (has_fgroups(p))
    return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_multinomial: feature groups (fos_feature_groups_bind) are bound; the group "
                                     "lasso over features serves the squared and the logistic loss");
  p->loss = FOS_LOSS_MULTINOMIAL;    // no buffer depends on the loss or on the number of classes: nothing to invalidate
  p->link_param = 0.0;
  p->classes = classes;
  return FOS_OK;
}

int fos_problem_get_classes(int* classes, const fos_problem* p) {
  if (!p || !classes) return fail(FOS_ERR_ARG, "fos_problem_get_classes: null");
  *classes = p->loss == FOS_LOSS_MULTINOMIAL ? p->classes : 0;
  return FOS_OK;
}

int fos_problem_get_loss(const fos_problem* p, int* loss) {
  if (!p || !loss) return fail(FOS_ERR_ARG, "fos_problem_get_loss: null");
  *loss = p->loss;
  return FOS_OK;
}

int fos_row_weights_bind(const float* w, fos_problem* p) {
  if (!p) return fail(FOS_ERR_ARG, "fos_row_weights_bind: null problem");
  if (((uintptr_t)w & 15) != 0) return fail(FOS_ERR_ARG, "fos_row_weights_bind: the weights are not 16-byte aligned");
  if (w) {
    if (!p->b) return fail(FOS_ERR_UNSUPPORTED, "fos_row_weights_bind: a weighted problem needs b");
    if (p->comm || p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, "fos_row_weights_bind: sharded problems are not served");
    if (!pair_dd_multi_supported(p))
      return fail(FOS_ERR_UNSUPPORTED, "fos_row_weights_bind: row weights run on the matrix-core pair (aligned streaming layout, "
                                       "65..16384 columns)");
  }
  p->row_weight = w;                 // no buffer depends on the weights: nothing to invalidate
  return FOS_OK;
}

int fos_row_weights_get(const float** w_out, const fos_problem* p) {
  if (!p || !w_out) return fail(FOS_ERR_ARG, "fos_row_weights_get: null");
  *w_out = p->row_weight;
  return FOS_OK;
}

int fos_coord_bind(const float* penalty_factor, const float* lower, const float* upper, fos_problem* p) {
  if (!p) return fail(FOS_ERR_ARG, "fos_coord_bind: null problem");
  if ((((uintptr_t)penalty_factor | (uintptr_t)lower | (uintptr_t)upper) & 15) != 0)
    return fail(FOS_ERR_ARG, "fos_coord_bind: a vector is not 16-byte aligned");
  if (penalty_factor || lower || upper) {
    if (!p->b) return fail(FOS_ERR_UNSUPPORTED, "fos_coord_bind: a problem with coordinate data needs b");
    if (p->comm || p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, "fos_coord_bind: sharded problems are not served");
    if (!pair_dd_multi_supported(p))
      return fail(FOS_ERR_UNSUPPORTED, "fos_coord_bind: penalty factors and bounds run on the matrix-core pair (aligned streaming "
                                       "layout, 65..16384 columns)");
    if (has_fgroups(p))
      return fail(FOS_ERR_UNSUPPORTED, "fos_coord_bind: feature groups (fos_feature_groups_bind) are bound; group weights cover the "
                                       "unpenalised coordinate, factors and bounds do not compose with the group norm");
  }
  p->coord_factor = penalty_factor;  // no buffer depends on the coordinate data: nothing to invalidate
  p->coord_lo = lower;
  p->coord_hi = upper;
  return FOS_OK;
}

int fos_coord_get(const float** penalty_factor, const float** lower, const float** upper, const fos_problem* p) {
  if (!p || !penalty_factor || !lower || !upper) return fail(FOS_ERR_ARG, "fos_coord_get: null");
  *penalty_factor = p->coord_factor;
  *lower = p->coord_lo;
  *upper = p->coord_hi;
  return FOS_OK;
}

// The table is checked on the host before any HIP call: a bad table never reaches a kernel.  What does not need the handle is
// checked first, so that a null handle and a malformed table are told apart without one.
int fos_feature_groups_bind(const int32_t* group_start, const float* group_weight, int32_t ngroups, double l1_mix, fos_problem* p) {
  if (!p) return fail(FOS_ERR_ARG, "fos_feature_groups_bind: null problem");
  const bool detach = ngroups == 0 && !group_start;
  if (!detach) {
    if (!group_start || ngroups < 1) return fail(FOS_ERR_ARG, "fos_feature_groups_bind: a table of ngroups >= 1 groups is needed");
    if (!(l1_mix >= 0.0 && l1_mix <= 1.0)) return fail(FOS_ERR_ARG, "fos_feature_groups_bind: l1_mix outside [0, 1]");
    if (group_start[0] != 0) return fail(FOS_ERR_ARG, "fos_feature_groups_bind: group_start[0] is not 0");
    for (int32_t g = 0; g < ngroups; ++g) {
      if (group_start[g + 1] <= group_start[g])
        return fail(FOS_ERR_ARG, "fos_feature_groups_bind: group_start is not strictly increasing at group " + std::to_string(g));
      if (group_weight && !(std::isfinite(group_weight[g]) && group_weight[g] >= 0.0f))
        return fail(FOS_ERR_ARG, "fos_feature_groups_bind: the weight of group " + std::to_string(g) + " is not finite and >= 0");
    }
    if ((int64_t)ngroups > p->n || (int64_t)group_start[ngroups] != p->n)
      return fail(FOS_ERR_ARG, "fos_feature_groups_bind: the groups do not partition the n = " + std::to_string(p->n) + " coordinates");
    if (!p->b) return fail(FOS_ERR_UNSUPPORTED, "fos_feature_groups_bind: a problem with feature groups needs b");
    if (p->comm || p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, "fos_feature_groups_bind: sharded problems are not served");
    if (!pair_dd_multi_supported(p))
      return fail(FOS_ERR_UNSUPPORTED, "fos_feature_groups_bind: feature groups run on the matrix-core pair (aligned streaming "
                                       "layout, 65..16384 columns)");
    if (has_coord(p))
      return fail(FOS_ERR_UNSUPPORTED, "fos_feature_groups_bind: penalty factors or bounds (fos_coord_bind) are bound; they do not "
                                       "compose with the group norm");
    if (p->loss == FOS_LOSS_MULTINOMIAL)
      return fail(FOS_ERR_UNSUPPORTED, "fos_feature_groups_bind: a multinomial problem is not served (squared and logistic loss)");
  }
  HIP_TRY(hipStreamSynchronize(p->stream));       // launches of an earlier binding may still read the buffers
  if (detach) {
    p->fg.reset();
    return FOS_OK;
  }
  const int64_t n4 = (p->n + 3) / 4 * 4;
  std::vector<float> w((size_t)ngroups);
  std::vector<int32_t> of_coord((size_t)n4, 0);
  for (int32_t g = 0; g < ngroups; ++g) {
    w[g] = group_weight ? group_weight[g] : std::sqrt((float)(group_start[g + 1] - group_start[g]));
    for (int32_t j = group_start[g]; j < group_start[g + 1]; ++j) of_coord[j] = g;
  }
  p->fg.ngroups = 0;                              // a failure below leaves the problem without feature groups
  int rc;
  if ((rc = p->fg.start.reserve((size_t)ngroups + 1)) || (rc = p->fg.weight.reserve((size_t)ngroups)) ||
      (rc = p->fg.of_coord.reserve((size_t)n4)) || (rc = p->fg.u.reserve((size_t)fos::BT_NV * n4)) ||
      (rc = p->fg.nrm2.reserve((size_t)fos::BT_NV * ngroups)))
    return rc;
  HIP_TRY(hipMemcpy(p->fg.start, group_start, ((size_t)ngroups + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->fg.weight, w.data(), (size_t)ngroups * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p->fg.of_coord, of_coord.data(), (size_t)n4 * sizeof(int32_t), hipMemcpyHostToDevice));
  p->fg.l1_mix = l1_mix;
  p->fg.ngroups = ngroups;
  return FOS_OK;
}

int fos_feature_groups_get(int32_t* ngroups, double* l1_mix, const fos_problem* p) {
  if (!p || !ngroups || !l1_mix) return fail(FOS_ERR_ARG, "fos_feature_groups_get: null");
  *ngroups = p->fg.ngroups;
  *l1_mix = p->fg.ngroups ? p->fg.l1_mix : 0.0;
  return FOS_OK;
}

int fos_problem_set_comm(fos_problem* p, fos_comm* c) {
  if (!p) return fail(FOS_ERR_ARG, "fos_problem_set_comm: null");
  if (int rc_ = need_squared(p, "fos_problem_set_comm")) return rc_;
  p->comm = c;
  return invalidate(p, IN_COMM);
}

int fos_problem_set_comm_cols(fos_problem* p, fos_comm* c) {
  if (!p || !c) return fail(FOS_ERR_ARG, "fos_problem_set_comm_cols: null");
  if (int rc_ = need_squared(p, "fos_problem_set_comm_cols")) return rc_;
  if (!vec_layout(p) || p->n <= tlr_max_n(p->dtype))
    return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_comm_cols: needs the streaming layout (aligned, more than 32 chunks of 16 bytes per row and rank)");
  // the two-phase column-block plan, whatever the width: r = sum_p A_p y_p - b is exchanged between the phases
  int64_t cb_width = 0;
  const MenuEntry* ce = colblock_entry(p, &cb_width);
  if (!ce) return fail(FOS_ERR_UNSUPPORTED, "fos_problem_set_comm_cols: no column-block kernel for this block width");
  p->comm = c;
  p->col_sharded = true;
  if (int rc = invalidate(p, IN_PLAN | IN_COMM)) return rc;
  p->pass.vec4 = true;
  plan_colblock(p, ce, cb_width);
  return ensure_workspace(p);
}

int fos_problem_set_stream(fos_problem* p, void* stream) {
  if (!p) return fail(FOS_ERR_ARG, "fos_problem_set_stream: null");
  hipStream_t ns = reinterpret_cast<hipStream_t>(stream);
  if (ns == p->stream) return FOS_OK;
  // work already enqueued on the old stream touches the handle's workspace: the new stream waits for it
  hipEvent_t ev;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, p->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(ns, ev, 0);
  (void)hipEventDestroy(ev);
  if (e != hipSuccess) return fail(FOS_ERR_HIP, std::string("fos_problem_set_stream: ") + hipGetErrorString(e));
  p->stream = ns;
  return FOS_OK;
}

int fos_problem_replan(fos_problem* p, unsigned flags) {
  if (!p) return fail(FOS_ERR_ARG, "fos_problem_replan: null");
  if (p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, "fos_problem_replan: a column-sharded problem keeps its two-phase plan");
  if (flags & ~(unsigned)(FOS_PLAN_NO_RESIDENT | FOS_PLAN_NO_TALL | FOS_PLAN_NO_WIDE | FOS_PLAN_NO_COLBLOCK | FOS_PLAN_CLUSTER |
                           FOS_PLAN_INTERLEAVE | FOS_PLAN_NO_INTERLEAVE | FOS_PLAN_NO_CLUSTER | FOS_PLAN_FUSED_MFMA |
                           FOS_PLAN_CHIP_RESIDENT | FOS_PLAN_NO_CHIP_RESIDENT | FOS_PLAN_PACK | FOS_PLAN_NO_PACK | FOS_PLAN_PACK_ROWS_MASK))
    return fail(FOS_ERR_ARG, "fos_problem_replan: unknown flag");
  const int pack_rows_req = (int)((flags & FOS_PLAN_PACK_ROWS_MASK) / FOS_PLAN_PACK_ROWS(1));
  if (pack_rows_req > (p->n <= 8192 ? 4 : 3))
    return fail(FOS_ERR_ARG, "fos_problem_replan: FOS_PLAN_PACK_ROWS takes 1 .. 4 rows per burst for n <= 8192 and 1 .. 3 above");
  p->cp_mode = (flags & FOS_PLAN_CLUSTER) ? 1 : (flags & FOS_PLAN_NO_CLUSTER) ? 2 : 0;
  p->fused_on = (flags & FOS_PLAN_FUSED_MFMA) != 0;
  p->chip_mode = (flags & FOS_PLAN_CHIP_RESIDENT) ? 1 : (flags & FOS_PLAN_NO_CHIP_RESIDENT) ? 2 : 0;
  p->pack_mode = (flags & FOS_PLAN_NO_PACK) ? 2 : (flags & FOS_PLAN_PACK) ? 1 : 0;
  flags &= ~(unsigned)(FOS_PLAN_CLUSTER | FOS_PLAN_NO_CLUSTER | FOS_PLAN_FUSED_MFMA | FOS_PLAN_CHIP_RESIDENT |
                       FOS_PLAN_NO_CHIP_RESIDENT | FOS_PLAN_PACK | FOS_PLAN_NO_PACK | FOS_PLAN_PACK_ROWS_MASK);
  int rc = invalidate(p, IN_PLAN);
  if (rc) return rc;
  p->pk.rows = pack_rows_req;                // lives with the copy: the next invalidating call puts the planner's back
  apply_plan(p, flags);
  return ensure_workspace(p);
}

int fos_stream_read_probe(const void* buf, size_t bytes, int launches, void* stream, double* gbps_out, double* us_out) {
  if (!buf || bytes < 16 || (bytes & 15) || (reinterpret_cast<uintptr_t>(buf) & 15) || launches < 1 || !gbps_out)
    return fail(FOS_ERR_ARG, "fos_stream_read_probe: needs a 16-byte aligned buffer of a multiple of 16 bytes and launches >= 1");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int dev = 0, ncu = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
  const size_t n16 = bytes / 16;
  const int grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)ncu, (n16 + 4095) / 4096));
  DevBuf<float> sink;
  if (int rc = sink.reserve((size_t)grid * 8)) return rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  // three orders - contiguous ranges per workgroup, one window swept by all in 8 KiB or in 64 KiB pieces - and the fastest one
  // counts: which of them leads depends on the size and on the state of the device (profiles/r03_row_order.md), as for the
  // product kernel
  float ms = 0.f;
  for (int order = 0; order < 3 && e == hipSuccess; ++order) {
    void (*kern)(const fos::f32x4*, size_t, float*) =
        order == 0 ? stream_read_kernel<0> : order == 1 ? stream_read_kernel<1> : stream_read_kernel<2>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), 0, st, (const fos::f32x4*)buf, n16, sink.get());      // warm-up
    e = hipEventRecord(e0, st);
    for (int i = 0; i < launches && e == hipSuccess; ++i) {
      hipLaunchKernelGGL(kern, dim3(grid), dim3(512), 0, st, (const fos::f32x4*)buf, n16, sink.get());
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float t = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    if (e == hipSuccess && (order == 0 || t < ms)) ms = t;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (e != hipSuccess) return fail(FOS_ERR_HIP, std::string("fos_stream_read_probe: ") + hipGetErrorString(e));
  const double us = (double)ms * 1e3 / launches;
  *gbps_out = (double)bytes / (us * 1e-6) / 1e9;
  if (us_out) *us_out = us;
  return FOS_OK;
}

int fos_problem_profile(fos_problem* p, int enable) {
  if (!p) return fail(FOS_ERR_ARG, "fos_problem_profile: null");
  p->profiling = enable > 0 ? enable : 0;
  p->prof_seq = 0;
  p->prof_open = false;
  return FOS_OK;
}

int fos_problem_profile_read(fos_problem* p, double* ms_total, int64_t* launches) {
  if (!p || !ms_total || !launches) return fail(FOS_ERR_ARG, "fos_problem_profile_read: null");
  int rc = prof_drain(p);
  if (rc) return rc;
  *ms_total = p->prof_ms;
  *launches = p->prof_launches;
  p->prof_ms = 0.0;
  p->prof_launches = 0;
  return FOS_OK;
}

int fos_problem_destroy(fos_problem* p) {
  if (!p) return FOS_OK;
  for (hipEvent_t e : p->ev_pool) (void)hipEventDestroy(e);
  delete p;
  return FOS_OK;
}

int fos_problem_plan(const fos_problem* p, int32_t plan[8]) {
  if (!p || !plan) return fail(FOS_ERR_ARG, "fos_problem_plan: null");
  plan[0] = p->pass.path;
  plan[1] = p->pass.entry ? p->pass.entry->threads : 256;
  plan[2] = p->pass.entry ? p->pass.entry->k : 0;
  plan[3] = p->pass.entry ? p->pass.entry->r : 0;
  plan[4] = p->pass.nwg;
  plan[5] = p->pass.nslabs;
  plan[6] = (p->pass.path == 0 ? 1 : 0) | (p->pass.resident ? 2 : 0) | (p->pass.tall ? 4 : 0) | (p->pass.colblock ? 8 : 0) | (p->multi.cp_cs ? 16 : 0) |
            ((p->il && p->pass.entry && p->pass.entry->with_g_il && p->pass.path == 0 && !p->pass.colblock && !p->pass.tall) ? 32 : 0) |
            (p->fused_on ? 64 : 0) | (p->chip_mode == 1 ? 128 : 0) | (p->pk.active ? 256 : 0) | ((pack_served(p) ? pack_rows(p) : 0) << 9);
  plan[7] = p->ncu;
  return FOS_OK;
}

int fos_problem_tune(fos_problem* p, int threads, int chunks, int rows, int workgroups) {
  if (!p) return fail(FOS_ERR_ARG, "fos_problem_tune: null");
  if (p->pass.path == 0 && p->pass.tall && workgroups > 0) {        // row-per-thread pass: only the workgroup count is tunable
    p->pass.rows_per_wg = ((p->m + workgroups - 1) / workgroups + 3) / 4 * 4;
    p->pass.nwg = (int)((p->m + p->pass.rows_per_wg - 1) / p->pass.rows_per_wg);
    p->pass.nslabs = p->pass.nwg;
    if (int rc = invalidate(p, IN_TUNE)) return rc;
    return ensure_workspace(p);
  }
  if (p->pass.path != 0 || p->pass.tall || p->pass.colblock)
    return fail(FOS_ERR_UNSUPPORTED, "fos_problem_tune: only the streaming single-pass kernel has a geometry menu");
  const MenuEntry* e = find_entry(p->dtype, threads, chunks, rows);
  if (!e || (int64_t)e->threads * e->k * epc_of(p->dtype) < p->n)
    return fail(FOS_ERR_UNSUPPORTED, "fos_problem_tune: geometry not instantiated or too narrow for n");
  plan_fused(p, e, workgroups);
  if (int rc = invalidate(p, IN_TUNE)) return rc;
  return ensure_workspace(p);
}

int fos_problem_tune_dd(fos_problem* p, int workgroups) {
  if (!p || workgroups < 0) return fail(FOS_ERR_ARG, "fos_problem_tune_dd: bad argument");
  if (p->pass.tall || p->pass.resident) return fail(FOS_ERR_UNSUPPORTED, "fos_problem_tune_dd: the tall / resident plans share the fp32 pass's grid");
  p->dd_nwg_hint = workgroups;
  return invalidate(p, IN_TUNE_DD);                // re-planned on the next fp64 pass (ensure_dd)
}

int fos_problem_set_gbuf(fos_problem* p, float* gbuf) {
  if (!p) return fail(FOS_ERR_ARG, "fos_problem_set_gbuf: null");
  if (gbuf && (reinterpret_cast<uintptr_t>(gbuf) & 15u)) return fail(FOS_ERR_ARG, "fos_problem_set_gbuf: misaligned");
  p->gbuf = gbuf ? gbuf : p->ws.gbuf_own;
  return FOS_OK;
}

int fos_gemv_pair(fos_problem* p, const float* y, float alpha2, float* grad, double* rr_out) {
  if (!p || !y || !grad) return fail(FOS_ERR_ARG, "fos_gemv_pair: null");
  if (int rc_ = need_squared(p, "fos_gemv_pair")) return rc_;
  const float* ya = nullptr;
  int rc = aligned_vec(p, y, &ya);
  if (rc) return rc;
  YSource ys{ya, nullptr, nullptr, nullptr, nullptr};
  int n_rr = 0;
  if ((rc = launch_pass(p, ys, p->b, true, &n_rr))) return rc;
  if ((rc = launch_slab_reduce(p, n_rr, p->gbuf, rr_out, nullptr))) return rc;
  hipLaunchKernelGGL(fos::add_l2_kernel<float>, dim3(grid_1d(p->n, 256, 1024)), dim3(256), 0, p->stream, p->gbuf,
                     (double)alpha2, ya, grad, p->n);
  LAUNCH_CHECK();
  return FOS_OK;
}

int fos_gemv_pair_f64(fos_problem* p, const double* y, double alpha2, float* grad, double* rr_out) {
  if (!p || !y || !grad) return fail(FOS_ERR_ARG, "fos_gemv_pair_f64: null");
  if (int rc_ = need_squared(p, "fos_gemv_pair_f64")) return rc_;
  if (p->pass.resident) {                           // small problem: one launch, fp64 throughout (resident.hpp)
    if (p->dtype == FOS_F32)
      hipLaunchKernelGGL(fos::gemv_pair_resident_kernel<float>, dim3(1), dim3(fos::RS_THREADS), 0, p->stream,
                         (const float*)p->A, p->lda, p->b, (int)p->m, (int)p->n, y, alpha2, grad, rr_out);
    else
      hipLaunchKernelGGL(fos::gemv_pair_resident_kernel<fos::bf16_t>, dim3(1), dim3(fos::RS_THREADS), 0, p->stream,
                         (const fos::bf16_t*)p->A, p->lda, p->b, (int)p->m, (int)p->n, y, alpha2, grad, rr_out);
    LAUNCH_CHECK();
    return FOS_OK;
  }
  YSource ys{nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, y};
  int n_rr = 0, rc;
  if ((rc = launch_pass(p, ys, p->b, true, &n_rr))) return rc;
  if ((rc = launch_slab_reduce(p, n_rr, p->gbuf, rr_out, nullptr))) return rc;
  hipLaunchKernelGGL(fos::add_l2_kernel<double>, dim3(grid_1d(p->n, 256, 1024)), dim3(256), 0, p->stream, p->gbuf, alpha2,
                     y, grad, p->n);
  LAUNCH_CHECK();
  return FOS_OK;
}

// The fp64-accumulating pass for any y source: out[0..n) = A^T (A y - b) + alpha2*l2vec (l2vec may be NULL when alpha2 = 0),
// out[n] = ||A y - b||^2, summed over the ranks of a sharded problem.  Not for resident-planned problems (callers check).
__global__ __launch_bounds__(256) void sumsq_f64_partials_kernel(const double* __restrict__ v, int64_t m, double* __restrict__ part,
                                                                const int* stopped) {
  if (stopped != nullptr && *stopped != 0) return;
  __shared__ double ws[4];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) acc += v[i] * v[i];
  acc = fos::wave_sum(acc);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}
__global__ __launch_bounds__(256) void unsum_f64_if_stopped_kernel(double* __restrict__ v, int64_t m, double scale, const int* stopped) {
  if (*stopped == 0) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) v[i] *= scale;
}

// Column-sharded form (fos_problem_set_comm_cols): this rank holds A[:, its columns] and its block of y.  Pass 1: the
// partial residual A_p y_p (rank 0 also subtracts b) in fp64, ONE all-reduce of the m doubles, pass 2: g_p = A_p^T r for
// the local block; alpha2*y_p is local.  out[0..n) is this rank's block of the gradient, out[n] the global ||r||^2.
static int launch_pass_dd_cols(fos_problem* p, const YSource& ys, double alpha2, const double* l2vec, double* out) {
  const float* b_here = p->comm->rank == 0 ? p->b : nullptr;
  int rc = launch_residual_rows(p, ys, b_here, p->dd.nwg, p->dd.rr);
  if (rc) return rc;
  if (ys.stopped != nullptr) {       // after a stop pass 1 was a no-op and rvec still holds the last SUM: divide it back
    hipLaunchKernelGGL(unsum_f64_if_stopped_kernel, dim3(grid_1d(p->m, 256, 1024)), dim3(256), 0, p->stream, p->pass.rvec, p->m,
                       1.0 / (double)p->comm->nranks, ys.stopped);
    LAUNCH_CHECK();
  }
  if ((rc = reduce_across(p, p->pass.rvec, (size_t)p->m, true))) return rc;
  const int n_rr = std::min(p->dd.nwg, 256);
  hipLaunchKernelGGL(sumsq_f64_partials_kernel, dim3(n_rr), dim3(256), 0, p->stream, p->pass.rvec, p->m, p->dd.rr, ys.stopped);
  LAUNCH_CHECK();
  if ((rc = launch_transpose_rows<double>(p, ys.stopped, p->dd.two_pass_chunks, p->dd.rows_per_wg, p->dd.slabs.get()))) return rc;
  hipLaunchKernelGGL(fos::slab_reduce_dd_kernel, dim3((unsigned)((p->n + fos::SRD_COLS - 1) / fos::SRD_COLS)),
                     dim3(fos::SRD_THREADS), 0, p->stream, p->dd.slabs, p->dd.two_pass_chunks, (int)p->n, (int64_t)p->n, p->dd.rr,
                     n_rr, alpha2, l2vec, out, ys.stopped);
  LAUNCH_CHECK();
  return FOS_OK;
}

}  // extern "C"
int fosapi::launch_pass_dd(fos_problem* p, const YSource& ys, double alpha2, const double* l2vec, double* out) {
  int rc = ensure_dd(p);
  if (rc) return rc;
  if (p->col_sharded) {
    if ((rc = prof_mark(p, true))) return rc;
    if ((rc = launch_pass_dd_cols(p, ys, alpha2, l2vec, out))) return rc;
    return prof_mark(p, false);
  }
  int nslabs = 0, n_rr = 0;
  int64_t stride = p->n;
  if ((rc = prof_mark(p, true))) return rc;
  if (p->pass.tall) {
    p->pass.entry->dd(p->A, p->lda, p->b, p->m, (int)p->n, ys, p->pass.rows_per_wg, p->dd.slabs, p->dd.rr, p->pass.nwg, p->stream);
    nslabs = n_rr = p->pass.nwg;
    stride = p->pass.slab_stride;
  } else if (p->dd.entry) {
    (p->il && p->dd.entry->fn_il ? p->dd.entry->fn_il : p->dd.entry->fn)(p->A, p->lda, p->b, p->m, (int)p->n, ys, p->dd.rows_per_wg, p->dd.slabs, p->dd.rr, p->dd.nwg, p->stream);
    nslabs = n_rr = p->dd.nwg;
  } else {
    if ((rc = launch_residual_rows(p, ys, p->b, p->dd.nwg, p->dd.rr)) ||
        (rc = launch_transpose_rows<double>(p, ys.stopped, p->dd.two_pass_chunks, p->dd.rows_per_wg, p->dd.slabs.get())))
      return rc;
    nslabs = p->dd.two_pass_chunks;
    n_rr = p->dd.nwg;
  }
  LAUNCH_CHECK();
  if ((rc = prof_mark(p, false))) return rc;
  // sharded: alpha2*x enters the sum over the ranks exactly once (rank 0 adds it to its partial)
  const double a2_here = (p->comm && p->comm->rank != 0) ? 0.0 : alpha2;
  hipLaunchKernelGGL(fos::slab_reduce_dd_kernel, dim3((unsigned)((p->n + fos::SRD_COLS - 1) / fos::SRD_COLS)),
                     dim3(fos::SRD_THREADS), 0, p->stream, p->dd.slabs,
                     nslabs, (int)p->n, stride, p->dd.rr, n_rr, a2_here, l2vec, out, p->comm ? nullptr : ys.stopped);
  LAUNCH_CHECK();
  return reduce_across(p, out, (size_t)p->n + 1, true);      // (sharded: re-derived after a stop, see launch_slab_reduce)
}
extern "C" {

int fos_gemv_pair_dd(fos_problem* p, const double* x, double alpha2, double* grad_rr) {
  if (!p || !x || !grad_rr) return fail(FOS_ERR_ARG, "fos_gemv_pair_dd: null");
  if (int rc_ = need_squared(p, "fos_gemv_pair_dd")) return rc_;
  return fosapi::gemv_pair_dd_stamped(p, x, alpha2, grad_rr, nullptr, nullptr);
}

}  // extern "C"
// fos_gemv_pair_dd; t_stamp (nullable): where the pass leaves the wall clock of its start, *stamped says whether the
// kernel that serves this plan does (the streaming fp64 kernel; the others leave it to the caller's stamp kernel)
int fosapi::gemv_pair_dd_stamped(fos_problem* p, const double* x, double alpha2, double* grad_rr, unsigned long long* t_stamp,
                                 bool* stamped) {
  if (stamped) *stamped = false;
  if (!p || !x || !grad_rr) return fail(FOS_ERR_ARG, "fos_gemv_pair_dd: null");
  if (p->pass.resident) {                           // small problem: one launch, fp64 throughout (resident.hpp)
    if (p->dtype == FOS_F32)
      hipLaunchKernelGGL((fos::gemv_pair_resident_kernel<float, double>), dim3(1), dim3(fos::RS_THREADS), 0, p->stream,
                         (const float*)p->A, p->lda, p->b, (int)p->m, (int)p->n, x, alpha2, grad_rr, grad_rr + p->n);
    else
      hipLaunchKernelGGL((fos::gemv_pair_resident_kernel<fos::bf16_t, double>), dim3(1), dim3(fos::RS_THREADS), 0,
                         p->stream, (const fos::bf16_t*)p->A, p->lda, p->b, (int)p->m, (int)p->n, x, alpha2, grad_rr,
                         grad_rr + p->n);
    LAUNCH_CHECK();
    return FOS_OK;
  }
  YSource ys{nullptr, nullptr, nullptr, nullptr, nullptr, 0.0, x};
  if (t_stamp != nullptr) {
    bool ok = false;
    int rc = dd_pass_stamps(p, &ok);
    if (rc) return rc;
    if (ok) ys.t_stamp = t_stamp;
    if (stamped) *stamped = ok;
  }
  return launch_pass_dd(p, ys, alpha2, x, grad_rr);
}
// whether the kernel behind fos_gemv_pair_dd on this plan writes YSource::t_stamp (the streaming fp64 kernel does)
int fosapi::dd_pass_stamps(fos_problem* p, bool* yes) {
  *yes = false;
  if (p->pass.resident) return FOS_OK;
  int rc = ensure_dd(p);
  if (rc) return rc;
  *yes = p->dd.entry != nullptr && !p->pass.tall && !p->col_sharded;
  return FOS_OK;
}
extern "C" {

int fos_residual_objective(fos_problem* p, const float* x, double* out3) {
  if (!p || !x || !out3) return fail(FOS_ERR_ARG, "fos_residual_objective: null");
  if (int rc_ = need_squared(p, "fos_residual_objective")) return rc_;
  const float* xa = nullptr;
  int rc = aligned_vec(p, x, &xa);
  if (rc) return rc;
  YSource ys{xa, nullptr, nullptr, nullptr, nullptr};
  int n_rr = 0;
  if ((rc = launch_pass(p, ys, p->b, false, &n_rr))) return rc;
  hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, p->pass.rr_part, n_rr, 1, out3);
  LAUNCH_CHECK();
  if (!p->col_sharded && (rc = reduce_across(p, out3, 1, true))) return rc;
  hipLaunchKernelGGL(fos::vec_norms_kernel, dim3(1), dim3(fos::LB_THREADS), 0, p->stream, xa, p->n, out3 + 1);
  LAUNCH_CHECK();
  if (p->col_sharded) return reduce_across(p, out3 + 1, 2, true);     // ||x||^2, ||x||_1 over the column blocks
  return FOS_OK;
}

// fos_residual_batch / _folds on the shapes of the matrix-core pair, in the form the problem and the fold mask ask for:
// out16[j] = sum r^2 or the sum of the log-loss of column j, weighted per row on a problem with row weights, over all rows or
// over the rows of the fold that column holds out.  Arguments are checked.
static int residual_batch_pair(fos_problem* p, const char* fn, const float* X, int nv, double* out16, const uint8_t* fold_of_row,
                               const fos::FoldHeld* held) {
  if (!pair_dd_multi_supported(p)) return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": the shape has no matrix-core pair");
  int rc = ensure_batch_workspace(p);
  if (rc) return rc;
  if ((rc = pack_candidates(p, X, nv))) return rc;
  BatchLaunch L{};
  L.b = p->b; L.use_b = 1; L.fold_of_row = fold_of_row; L.held = held; L.row_weight = p->row_weight;
  return residual_batch_sums(p, L, out16);
}

// fos_residual_batch / _folds on a multinomial problem: per row panel the storing product 1 in its plain form (the logits of
// the panel in rbuf16), then the link kernel (softmax_link.hpp), whose partials of all panels fold into out16: out16[s * C] =
// the loss sum of segment s, weighted per row on a problem with row weights, over all rows (held == nullptr) or over the rows
// of the fold the segment holds out; 0 in the other entries.  Arguments are checked.
static int residual_batch_softmax(fos_problem* p, const char* fn, const float* X, int nv, double* out16, const uint8_t* fold_of_row,
                                  const fos::FoldHeld* held) {
  if (!pair_dd_multi_supported(p)) return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": the shape has no matrix-core pair");
  int rc = ensure_batch_workspace(p);
  if (rc) return rc;
  if ((rc = plan_multi_mfma(p))) return rc;
  const int64_t panels = (p->m + p->multi.panel_rows - 1) / p->multi.panel_rows;
  if ((rc = p->ws.link_part.reserve((size_t)panels * p->ncu * fos::BT_NV))) return rc;
  if ((rc = pack_candidates(p, X, nv))) return rc;
  const int64_t esz = p->dtype == FOS_BF16 ? 2 : 4;
  int nparts = 0;
  for (int64_t row0 = 0; row0 < p->m; row0 += p->multi.panel_rows) {
    const int64_t rows = std::min<int64_t>(p->multi.panel_rows, p->m - row0);
    int nwg1 = 0, nwg = 0;
    BatchLaunch L{};                 // Z = A_panel X: no b, no mask, no weights
    L.A = reinterpret_cast<const char*>(p->A) + (size_t)row0 * p->lda * esz; L.rows = rows; L.rout = p->multi.rbuf16;
    if ((rc = launch_batch_product(p, L, &nwg1))) return rc;
    if ((rc = launch_softmax_link(p, row0, rows, nv, held ? fos::FOLD_HELD : fos::FOLD_OFF, fold_of_row, held,
                                  p->ws.link_part + (size_t)nparts * fos::BT_NV, &nwg)))
      return rc;
    nparts += nwg;
  }
  hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, p->ws.link_part, nparts, fos::BT_NV, out16);
  LAUNCH_CHECK();
  return FOS_OK;
}

// ... and on a Huber or squared-hinge problem: the same with the pointwise link kernel (pointwise_link.hpp), any nv in 1..16:
// out16[j] = the data term of column j (its 1/2 included), weighted per row on a problem with row weights, over all rows or over
// the rows of the fold that column holds out.
static int residual_batch_link(fos_problem* p, const char* fn, const float* X, int nv, double* out16, const uint8_t* fold_of_row,
                               const fos::FoldHeld* held) {
  if (!pair_dd_multi_supported(p)) return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": the shape has no matrix-core pair");
  int rc = ensure_batch_workspace(p);
  if (rc) return rc;
  if ((rc = plan_multi_mfma(p))) return rc;
  const int64_t panels = (p->m + p->multi.panel_rows - 1) / p->multi.panel_rows;
  if ((rc = p->ws.link_part.reserve((size_t)panels * 2 * p->ncu * fos::BT_NV))) return rc;
  if ((rc = pack_candidates(p, X, nv))) return rc;
  const int64_t esz = p->dtype == FOS_BF16 ? 2 : 4;
  int nparts = 0;
  for (int64_t row0 = 0; row0 < p->m; row0 += p->multi.panel_rows) {
    const int64_t rows = std::min<int64_t>(p->multi.panel_rows, p->m - row0);
    int nwg1 = 0, nwg = 0;
    BatchLaunch L{};                 // Z = A_panel X: no b, no mask, no weights
    L.A = reinterpret_cast<const char*>(p->A) + (size_t)row0 * p->lda * esz; L.rows = rows; L.rout = p->multi.rbuf16;
    if ((rc = launch_batch_product(p, L, &nwg1))) return rc;
    if ((rc = launch_pointwise_link(p, row0, rows, nv, held ? fos::FOLD_HELD : fos::FOLD_OFF, fold_of_row, held,
                                    p->ws.link_part + (size_t)nparts * fos::BT_NV, &nwg)))
      return rc;
    nparts += nwg;
  }
  hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, p->ws.link_part, nparts, fos::BT_NV, out16);
  LAUNCH_CHECK();
  return FOS_OK;
}

int fos_residual_batch(fos_problem* p, const float* X, int nv, int use_b, double* out16) {
  if (!p || !X || !out16 || nv < 1 || nv > fos::BT_NV) return fail(FOS_ERR_ARG, "fos_residual_batch: bad argument");
  if (!use_b)                        // ||A X_j||^2 is a squared-loss quantity
    if (int rc = need_squared(p, "fos_residual_batch (use_b = 0)")) return rc;
  if (p->loss == FOS_LOSS_MULTINOMIAL) {
    if (!softmax_groups_ok(p, nv, nullptr)) return fail(FOS_ERR_ARG, "fos_residual_batch: on a multinomial problem nv is a multiple of the classes");
    return residual_batch_softmax(p, "fos_residual_batch", X, nv, out16, nullptr, nullptr);
  }
  if (link_loss(p)) return residual_batch_link(p, "fos_residual_batch", X, nv, out16, nullptr, nullptr);
  if (p->loss == FOS_LOSS_LOGISTIC || p->row_weight) return residual_batch_pair(p, "fos_residual_batch", X, nv, out16, nullptr, nullptr);
  if (!batch_supported(p)) return fail(FOS_ERR_UNSUPPORTED, "fos_residual_batch: needs the fused path");
  int rc = ensure_batch_workspace(p);
  if (rc) return rc;
  if ((rc = pack_candidates(p, X, nv))) return rc;
  return launch_residual_batch(p, use_b, out16);
}

int fos_residual_batch_rhs(fos_problem* p, const float* X, int nv, const float* B, int64_t ldb, double* out16) {
  if (!p || !X || !B || !out16 || nv < 1 || nv > fos::BT_NV || ldb < nv)
    return fail(FOS_ERR_ARG, "fos_residual_batch_rhs: bad argument (null pointer, nv outside 1..16 or ldb < nv)");
  if (int rc_ = need_squared(p, "fos_residual_batch_rhs")) return rc_;
  if (p->comm || p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, "fos_residual_batch_rhs: sharded problems are not served");
  if (!batch_supported(p)) return fail(FOS_ERR_UNSUPPORTED, "fos_residual_batch_rhs: needs the fused path");
  int rc = ensure_batch_workspace(p);
  if (rc) return rc;
  if ((rc = stage_b16(p, B, ldb, nv))) return rc;
  if ((rc = pack_candidates(p, X, nv))) return rc;
  return launch_residual_batch(p, 1, out16, nullptr, p->ws.b16);
}

int fos_residual_batch_folds(fos_problem* p, const float* X, int nv, const uint8_t* fold_of_row, const int32_t* held,
                             double* out16) {
  fos::FoldHeld hb{};
  if (!p || !X || !fold_of_row || !held || !out16 || nv < 1 || nv > fos::BT_NV || ((uintptr_t)fold_of_row & 3) != 0 ||
      !fold_held_block(held, nv, &hb))
    return fail(FOS_ERR_ARG, "fos_residual_batch_folds: bad argument (null pointer, nv outside 1..16, fold_of_row not 4-byte "
                             "aligned or a held id outside -1..254)");
  if (!p->b) return fail(FOS_ERR_UNSUPPORTED, "fos_residual_batch_folds: the problem has no b of its own");
  if (p->comm || p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, "fos_residual_batch_folds: sharded problems are not served");
  if (p->loss == FOS_LOSS_MULTINOMIAL) {
    if (!softmax_groups_ok(p, nv, held))
      return fail(FOS_ERR_ARG, "fos_residual_batch_folds: on a multinomial problem nv is a multiple of the classes and the columns of "
                               "a class group hold out one fold");
    return residual_batch_softmax(p, "fos_residual_batch_folds", X, nv, out16, fold_of_row, &hb);
  }
  if (link_loss(p)) return residual_batch_link(p, "fos_residual_batch_folds", X, nv, out16, fold_of_row, &hb);
  return residual_batch_pair(p, "fos_residual_batch_folds", X, nv, out16, fold_of_row, &hb);
}

int fos_gemv_pair_dd_multi(fos_problem* p, const double* X, int nv, int64_t ldx, const float* B, int64_t ldb, double alpha2,
                           double* G, double* rr) {
  if (!p || !X || !B || !G || !rr || nv < 1 || nv > fos::BT_NV || ldb < nv || ldx < 1)
    return fail(FOS_ERR_ARG, "fos_gemv_pair_dd_multi: bad argument (null pointer, nv outside 1..16, ldb < nv or ldx < n)");
  if (ldx < p->n) return fail(FOS_ERR_ARG, "fos_gemv_pair_dd_multi: bad argument (ldx < n)");
  if (int rc_ = need_squared(p, "fos_gemv_pair_dd_multi")) return rc_;
  if (!pair_dd_multi_supported(p)) return pair_dd_multi(p, fos::DdMultiCols{}, 0, 0u, alpha2, nullptr);
  fos::DdMultiCols c{};
  for (int j = 0; j < nv; ++j) {
    c.x[j] = X + (size_t)j * ldx;
    c.g[j] = G + (size_t)j * ldx;
    c.rr[j] = rr + j;
    c.col[j] = j;
  }
  int rc = stage_b16(p, B, ldb, nv);
  if (rc) return rc;
  return pair_dd_multi(p, c, nv, (1u << nv) - 1u, alpha2, p->ws.b16);
}

int fos_power_iter(fos_problem* p, float* v_inout, int n_iter, double tol, double* L_out, int* iters_out) {
  if (!p || !v_inout || !L_out || n_iter <= 0) return fail(FOS_ERR_ARG, "fos_power_iter: bad argument");
  if (p->col_sharded)
    return fail(FOS_ERR_UNSUPPORTED, "fos_power_iter: column-sharded problems normalise over the ranks (see _lipschitz_cols)");
  // L after every step (+ the norm of v0): sized by the caller's n_iter
  if (int rc = p->ws.lhist.reserve((size_t)n_iter + 1)) return rc;
  double* Lh = p->ws.lhist;        // n_iter + 1 slots
  if (p->pass.resident) {
    // all iterations in one launch; the break rule (:57) is evaluated on the device
    int* used_dev = reinterpret_cast<int*>(p->ws.dscal + 240);
    if (p->dtype == FOS_F32)
      hipLaunchKernelGGL(fos::power_resident_kernel<float>, dim3(1), dim3(fos::RS_THREADS), 0, p->stream,
                         (const float*)p->A, p->lda, (int)p->m, (int)p->n, v_inout, n_iter, tol, Lh, used_dev);
    else
      hipLaunchKernelGGL(fos::power_resident_kernel<fos::bf16_t>, dim3(1), dim3(fos::RS_THREADS), 0, p->stream,
                         (const fos::bf16_t*)p->A, p->lda, (int)p->m, (int)p->n, v_inout, n_iter, tol, Lh, used_dev);
    LAUNCH_CHECK();
    std::vector<double> hL(n_iter);
    int used = 0;
    HIP_TRY(hipMemcpyAsync(&used, used_dev, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(hL.data(), Lh, (size_t)n_iter * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (used < 1 || used > n_iter) return fail(FOS_ERR_HIP, "fos_power_iter: resident kernel returned no result");
    *L_out = hL[used - 1];
    if (iters_out) *iters_out = used;
    return FOS_OK;
  }
  // The iterate after step `it` lives in slot it % 16 of a ring of 16 vectors (16-byte aligned slots), so that the one
  // the break rule selects is still there when the chunk that ran past it has been read back; v0 / ||v0|| takes the
  // slot step 0 reads, the last one.
  const int chunk = 16;
  const size_t vstride = ((size_t)p->n + 3) & ~(size_t)3;
  if (int rc = p->ws.vring.reserve((size_t)chunk * vstride)) return rc;
  float* ring = p->ws.vring;
  auto slot = [&](int it) { return ring + (size_t)((it + chunk) % chunk) * vstride; };
  // v = v0 / ||v0||   (iterative_solvers.py:51)
  hipLaunchKernelGGL(fos::power_normalize_kernel, dim3(1), dim3(1024), 0, p->stream, v_inout, (int)p->n, slot(-1),
                     Lh + n_iter);
  LAUNCH_CHECK();
  // The reference breaks as soon as |L - prev| < tol (:57).  The iterations are enqueued in chunks; after each chunk
  // the L values are read back and the break rule is replayed on the host, so a matrix with a dominant eigenvalue
  // stops after a chunk instead of running all n_iter passes (L, the step and v are those of the step that broke).
  std::vector<double> hL(n_iter);
  double prev = 0.0;
  int used = n_iter, done = 0;
  bool hit = false;
  while (done < n_iter && !hit) {
    const int todo = std::min(chunk, n_iter - done);
    for (int it = done; it < done + todo; ++it) {
      YSource ys{slot(it - 1), nullptr, nullptr, nullptr, nullptr};
      int n_rr = 0, rc;
      if ((rc = launch_pass(p, ys, nullptr, true, &n_rr))) return rc;                       // w = A^T (A v)   :54
      if ((rc = launch_slab_reduce(p, n_rr, p->gbuf, nullptr, nullptr))) return rc;
      hipLaunchKernelGGL(fos::power_normalize_kernel, dim3(1), dim3(1024), 0, p->stream, p->gbuf, (int)p->n, slot(it),
                         Lh + it);                                                         // L = ||w||, v = w/L :55-56
      LAUNCH_CHECK();
    }
    HIP_TRY(hipMemcpyAsync(hL.data() + done, Lh + done, (size_t)todo * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    for (int it = done; it < done + todo; ++it) {      // |L - prev| < tol -> break   :57
      if (std::fabs(hL[it] - prev) < tol) { used = it + 1; hit = true; break; }
      prev = hL[it];
    }
    done += todo;
  }
  // the iterate after `used` steps: the one L_out and iters_out belong to
  HIP_TRY(hipMemcpyAsync(v_inout, slot(used - 1), (size_t)p->n * sizeof(float), hipMemcpyDeviceToDevice, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  *L_out = hL[used - 1];
  if (iters_out) *iters_out = used;
  return FOS_OK;
}

int fos_prox_l1(const float* v, float thr, float* out, int64_t n, void* stream) {
  if (n == 0) return FOS_OK;
  if (!v || !out || n < 0) return fail(FOS_ERR_ARG, "fos_prox_l1: bad argument");
  hipLaunchKernelGGL(fos::prox_l1_kernel, dim3(grid_1d(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, v, thr, out, n);
  LAUNCH_CHECK();
  return FOS_OK;
}

int fos_prox_l1_vec(const float* v, const float* thr, float* out, int64_t n, void* stream) {
  if (n == 0) return FOS_OK;
  if (!v || !thr || !out || n < 0) return fail(FOS_ERR_ARG, "fos_prox_l1_vec: bad argument");
  hipLaunchKernelGGL(fos::prox_l1_vec_kernel, dim3(grid_1d(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, v, thr, out, n);
  LAUNCH_CHECK();
  return FOS_OK;
}

int fos_prox_elastic_net(const float* v, float tau, float alpha1, float alpha2, float* out, int64_t n, void* stream) {
  if (n == 0) return FOS_OK;
  if (!v || !out || n < 0) return fail(FOS_ERR_ARG, "fos_prox_elastic_net: bad argument");
  hipLaunchKernelGGL(fos::prox_enet_kernel, dim3(grid_1d(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, v, tau,
                     alpha1, alpha2, out, n);
  LAUNCH_CHECK();
  return FOS_OK;
}

int fos_prox_elastic_net_vec(const float* v, const float* tau, float alpha1, float alpha2, float* out, int64_t n,
                             void* stream) {
  if (n == 0) return FOS_OK;
  if (!v || !tau || !out || n < 0) return fail(FOS_ERR_ARG, "fos_prox_elastic_net_vec: bad argument");
  hipLaunchKernelGGL(fos::prox_enet_vec_kernel, dim3(grid_1d(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, v, tau,
                     alpha1, alpha2, out, n);
  LAUNCH_CHECK();
  return FOS_OK;
}

// One power iteration per problem of a batch, one workgroup each (resident_batch.hpp).
int fos_power_iter_batch(const void* A, int a_dtype, const fos_batch_item* items, int count, float* v_inout, int64_t ldv,
                         int n_iter, double tol, double* L_out, int32_t* iters_used, void* work, void* stream) {
  if (count < 0 || n_iter < 1 || (a_dtype != FOS_F32 && a_dtype != FOS_BF16))
    return fail(FOS_ERR_ARG, "fos_power_iter_batch: bad argument (count < 0, n_iter < 1 or a_dtype)");
  if (count == 0) return FOS_OK;
  if (!A || !items || !v_inout || !L_out || !iters_used || !work || ldv < 1)
    return fail(FOS_ERR_ARG, "fos_power_iter_batch: bad argument (null pointer or ldv < 1)");
  if (int rc = check_batch_items("fos_power_iter_batch", items, count, ldv)) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  auto* dev_items = reinterpret_cast<fos_batch_item*>(work);
  HIP_TRY(hipMemcpyAsync(dev_items, items, (size_t)count * sizeof(fos_batch_item), hipMemcpyHostToDevice, st));
  if (a_dtype == FOS_F32)
    hipLaunchKernelGGL(fos::power_resident_batch_kernel<float>, dim3(count), dim3(fos::RS_THREADS), 0, st,
                       (const float*)A, dev_items, v_inout, ldv, n_iter, tol, L_out, iters_used);
  else
    hipLaunchKernelGGL(fos::power_resident_batch_kernel<fos::bf16_t>, dim3(count), dim3(fos::RS_THREADS), 0, st,
                       (const fos::bf16_t*)A, dev_items, v_inout, ldv, n_iter, tol, L_out, iters_used);
  LAUNCH_CHECK();
  return FOS_OK;
}

}  // extern "C"
