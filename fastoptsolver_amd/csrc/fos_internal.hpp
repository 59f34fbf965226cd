// Internal header of libfos_hip.so: the handle types behind include/fos.h and the launch helpers shared by the translation
// units of the C ABI (fos_plan.hip: planner, kernel menus, problem-level entry points; fos_comm.hip: communicators;
// fos_fista.hip: the FISTA state machine; fos_lbfgs.hip: L-BFGS).  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <chrono>
#include <vector>

// the library is built with -fvisibility=hidden: only what include/fos.h declares is exported
#pragma GCC visibility push(default)
#include "../../include/fos.h"
#include "../../include/fos_feature_groups.h"
#include "../../include/fos_link_loss.h"
#include "../../include/fos_working_set.h"
#include "../../include/fos_duality.h"
#include "../../include/fos_multinomial_ws.h"
#include "../../include/fos_resample.h"
#pragma GCC visibility pop
#include "batch_trial.hpp"
#include "cluster_pass.hpp"
#include "comm.hpp"
#include "gemv_multi.hpp"
#include "gemv_pair.hpp"
#include "gemv_tall.hpp"
#include "gemv_wide.hpp"
#include "gram_batch.hpp"
#include "gram_batch_dd.hpp"
#include "lbfgs_driver.hpp"
#include "lbfgs_kernels.hpp"
#include "reduce_update.hpp"
#include "resident.hpp"
#include "resident_batch.hpp"


namespace fosapi {

extern thread_local std::string g_err;            // fos_last_error(): per-thread text of the last failure

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return fail(FOS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                      \
  } while (0)
#define LAUNCH_CHECK()                                                                                  \
  do {                                                                                                  \
    hipError_t e_ = hipGetLastError();                                                                  \
    if (e_ != hipSuccess) return fail(FOS_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e_)); \
  } while (0)

// The one owner of an allocation the library makes: freed once (in the destructor or in reset(), with a plain hipFree, which
// waits for the device), sized in BYTES.  Every device buffer of a handle is a DevBuf member; a raw pointer member is memory
// that belongs to the caller.  Converts to the raw pointer for kernel arguments.  PINNED: host memory the device can write.
template <class T, bool PINNED = false>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : ptr_(o.ptr_), bytes_(o.bytes_) { o.ptr_ = nullptr; o.bytes_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      std::swap(ptr_, o.ptr_);
      std::swap(bytes_, o.bytes_);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (ptr_) (void)(PINNED ? hipHostFree(ptr_) : hipFree(ptr_));
    ptr_ = nullptr;
    bytes_ = 0;
  }
  // Room for `count` elements: a no-op when the buffer is large enough, otherwise freed and allocated to exactly
  // count * sizeof(T) bytes (contents are not kept).  A failed allocation leaves the buffer empty: the next call tries again.
  int reserve(size_t count) {
    const size_t need = count * sizeof(T);
    if (ptr_ && need <= bytes_) return FOS_OK;
    reset();
    const hipError_t e = PINNED ? hipHostMalloc(&ptr_, need) : hipMalloc(&ptr_, need);
    if (e != hipSuccess) {
      ptr_ = nullptr;
      return fail(FOS_ERR_HIP, std::string(PINNED ? "hipHostMalloc(" : "hipMalloc(") + std::to_string(need) + " bytes): " +
                                   hipGetErrorString(e));
    }
    bytes_ = need;
    return FOS_OK;
  }
  T* get() const { return ptr_; }
  operator T*() const { return ptr_; }
  T* operator->() const { return ptr_; }

 private:
  T* ptr_ = nullptr;
  size_t bytes_ = 0;
};
template <class T>
using PinnedBuf = DevBuf<T, true>;

using fos::YSource;

typedef void (*FusedLaunch)(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw,
                            float* slabs, double* rr_part, double* rr2_part, int nwg, hipStream_t st);

typedef void (*FusedLaunchDD)(const void* A, int64_t lda, const float* b, int64_t m, int n, YSource ys, int64_t rpw,
                              double* slabs, double* rr_part, int nwg, hipStream_t st);
struct MenuEntry {
  int dtype, threads, k, r;
  FusedLaunch with_g, resid_only, dual;   // dual may be null (geometry without a DUAL instantiation)
  FusedLaunchDD dd;                       // tall entries only: the same kernel writing fp64 slabs
  // column-block instantiations (CB = true: negated-residual store + slab stride), only on the two geometries a column
  // block can land on (block widths lie in (8192, 16384]); null elsewhere
  FusedLaunch with_g_cb = nullptr, resid_only_cb = nullptr;
  // interleaved-rows instantiations (IL = true: rows dealt round-robin, all CUs stream ONE contiguous window), on the
  // geometries of rows >= 16 KiB; null elsewhere
  FusedLaunch with_g_il = nullptr, resid_only_il = nullptr, dual_il = nullptr;
};
// Streaming geometries of the fp64-accumulating pass, ordered by capacity.  y and the gradient slice cost two VGPRs
// per column here, so the wide rows take 512 threads x 8 chunks (2 waves per SIMD, 256 VGPRs) instead of 1024 x 4.
struct DdEntry { int dtype, threads, k, r; FusedLaunchDD fn; FusedLaunchDD fn_il = nullptr; };
typedef void (*MultiLaunch)(const float* A, int64_t lda, const float* b, int64_t m, int n, fos::MultiY ys, int64_t rpw,
                            float* slabs, double* rr_part, int nwg, hipStream_t st);
}  // namespace fosapi

using fosapi::MenuEntry;
using fosapi::DdEntry;

using fosapi::DevBuf;
using fosapi::PinnedBuf;

// Device + pinned workspace of fos_lbfgs_minimize, cached on the problem handle (allocating per fit cost more than an 8 ms
// fit's iterations, and the frees at its end drain the device).  Complete only when n is set.
struct LbfgsWork {
  int64_t n = 0;
  DevBuf<double> g, g_old, d, x_old, S, Y, vl;
  PinnedBuf<double> host;              // 16 doubles
  DevBuf<unsigned long long> t_start;  // wall-clock stamp taken in front of an evaluation
  double ticks_per_ms = 1e5;           // hipDeviceAttributeWallClockRate (kHz)
  bool pass_stamps = false;           // the pass kernel of this plan stamps its own start (dd_pass_stamps)
};

// Device + pinned workspace of fos_lbfgs_minimize_multi (16 columns, column-contiguous), cached like LbfgsWork.
struct LbfgsMultiWork {
  int64_t n = 0;
  DevBuf<double> g;                    // [2][16][n]: the two gradient buffers of every column (current / previous)
  DevBuf<double> d, x_old, S, Y, vl, rr;
  PinnedBuf<double> host;              // 16 columns x 16 doubles, then the sequence number
  DevBuf<unsigned> count;              // workgroups of the statistics launch that have reported
  DevBuf<unsigned long long> t_start;
  double ticks_per_ms = 1e5;
};

// The plan of a problem handle, in groups: each holds the numbers of ONE decision and the buffers that decision sizes, names
// the inputs it was derived from, and is cleared as a whole by reset().  fosapi::invalidate (fos_plan.hip) is the one place
// that decides which groups an entry point resets; a group is rebuilt by its planner function on the next use.

// fp32 pass.  From: shape, layout (lda, alignment of A), plan flags, fos_problem_tune, comm (resident), column sharding.
// Filled by apply_plan / plan_cols (plan_fused, plan_tall, plan_fallback, plan_resident), buffers by ensure_workspace; the
// fused step and the multi-vector VALU pass reserve more slabs / partials for their own grids.
struct PassPlan {
  int path = 0;                      // 0 fused, 1 two-pass fallback
  bool resident = false;             // small enough for the single-launch LDS-resident loop (resident.hpp)
  bool tall = false;                 // n <= 64: row-per-thread single pass (gemv_tall.hpp); no alignment requirements
  // Rows wider than one workgroup's registers / LDS (fp32 > 32768 columns, bf16 > 16384): column blocks of cb_width
  // columns through the streaming kernel in two phases, r = A y - b block by block, then A^T r block by block
  bool colblock = false;
  int64_t cb_width = 0;
  int64_t slab_stride = 0;           // floats between slab rows (0 = n); the tall pass pads rows to a multiple of 4
  bool vec4 = false;                 // n % 4 == 0: float4 epilogues
  const MenuEntry* entry = nullptr;
  int nwg = 0;                       // workgroups of the fused kernel
  int nslabs = 0;
  int64_t rows_per_wg = 0;
  int resid_grid = 0;                // fallback pass-1 grid
  DevBuf<float> slabs;
  DevBuf<double> rr_part;
  DevBuf<double> rr2_part;           // DUAL pass: partials of ||A x_k - b||^2
  DevBuf<double> rvec;               // two-pass forms (this one and the fp64 pass's): residual (m doubles)
  DevBuf<float> rneg;                // m floats: the negated residual between the two column-block phases
  DevBuf<float> zeros;               // cb_width floats of zeros (phase 2 runs the same kernel with y = 0, b = -r)
  void reset() { *this = PassPlan{}; }
};

// fp64-accumulating pass (fos_gemv_pair_dd).  From: the fp32 pass group (tall plans share its grid and slab stride; resident
// plans need nothing), dd_nwg_hint, column sharding.  Filled by ensure_dd on first use.
struct DdPlan {
  bool planned = false;
  const DdEntry* entry = nullptr;    // streaming geometry; null: tall (the fp32 pass's entry) or two-pass
  int nwg = 0;
  int64_t rows_per_wg = 0;
  int two_pass_chunks = 0;           // > 0: this shape runs the fp64 two-pass kernels for the dd pass
  DevBuf<double> slabs;
  DevBuf<double> rr;
  void reset() { *this = DdPlan{}; }
};

// Multi-weight lockstep on the matrix cores (gram_batch.hpp; one-read form: cluster_pass.hpp).  From: shape, cp_mode, comm,
// col_sharded, the communicator's inbox size.  Filled by plan_multi_mfma on first use.
struct MultiPlan {
  bool planned = false;
  int64_t panel_rows = 0;
  int gram_splits = 0;
  int64_t gram_rows_per_split = 0;
  int cp_cs = 0, cp_clusters = 0;    // members per cluster (0: two products per panel), clusters
  int64_t cp_rows_per_cluster = 0;
  DevBuf<float> rbuf16;              // residual panel: panel_rows x 16 floats
  DevBuf<float> slabs16;             // the 16 gradient slab sets: splits x 16 x n floats
  DevBuf<float> cp_xchg;             // one-read form: hand-off ring
  DevBuf<unsigned> cp_flags;         // zeroed when allocated; fos_problem::cp_epoch keeps counting across a rebuild
  DevBuf<int> cp_error;
  void reset() { *this = MultiPlan{}; }
};

// fp64 multi-point pass on the matrix cores (gram_batch_dd.hpp, fos_gemv_pair_dd_multi).  From: shape, CU count.  Filled by
// ensure_dd_multi on first use.
struct DdMultiPlan {
  bool planned = false;
  int64_t n_pad = 0, panel_rows = 0, rows_per_split = 0;
  int splits = 0;
  DevBuf<double> xd;                 // staged points: n_pad x 16 doubles (Xp layout)
  DevBuf<double> rdd;                // residual panel: panel_rows x 16 doubles
  DevBuf<double> slabs;              // splits x 16 x n doubles
  DevBuf<double> q_part;             // product-1 partials of all panels: panels x 2 * ncu x 16 doubles
  void reset() { *this = DdMultiPlan{}; }
};

// Candidate block of the batched (MFMA) residual and of the lockstep.  From: shape, dtype, CU count.  Filled by
// ensure_batch_workspace on first use.
struct CandPlan {
  bool planned = false;
  int64_t n_pad = 0;
  DevBuf<float> xp;                  // permuted candidate block (bf16 storage: three bf16 terms per entry)
  DevBuf<double> q_part;             // per-workgroup partials
  DevBuf<double> bt_out;             // folded results: 128 doubles
  void reset() { *this = CandPlan{}; }
};

// 28-bit packed copy of an fp32 A for the gradient pass (gemv_packed.hpp).  From: A's contents at pack time, shape, the fp32
// pass group (streaming single pass, its grid and row order are reused), pack_mode, free device memory.  Filled by
// ensure_packed on the first call of the fos_fista_run family; `tried` keeps a refused matrix from being examined again.
struct PackPlan {
  bool tried = false, active = false;
  int threads = 0;                   // geometry the rows are laid out for: 1024 (n <= 16384) or 512 (n <= 8192)
  int rows = 0;                      // rows per burst of the pass: FOS_PLAN_PACK_ROWS(1 .. 4) of the replan that made this plan,
                                     // 0: the planner's for the geometry and row order (pack_rows); dropped with the copy
  unsigned e0 = 0;                   // first biased exponent of the 16-binade window (even)
  int64_t nnz = 0;                   // out-of-window elements
  DevBuf<unsigned char> P;           // m rows of pk::row_bytes(threads)
  DevBuf<int> csr_ptr, csr_col, csc_ptr, csc_row;       // D = A - P, row-sorted and column-sorted
  DevBuf<float> csr_tv, csr_pv, csc_tv, csc_pv;         // per exception: the true value and the stored placeholder
  DevBuf<float> bprime, r;           // m floats each: b - D y, and the residual the pass stores
  void reset() { *this = PackPlan{}; }
};

// Feature groups of the lockstep's update (fos_feature_groups_bind; reduce_update.hpp).  From: the caller's table alone - no plan
// input enters, so fosapi::invalidate leaves the group as it is; a second bind overwrites it, a detaching bind and the
// destruction of the problem reset it.  Filled by fos_feature_groups_bind, which reserves everything once.
struct FeatureGroups {
  int32_t ngroups = 0;               // 0: none bound
  double l1_mix = 0.0;
  DevBuf<int32_t> start;             // ngroups + 1 boundaries
  DevBuf<float> weight;              // ngroups weights
  DevBuf<int32_t> of_coord;          // the group of every coordinate: n rounded up to 4 entries
  DevBuf<double> u;                  // 16 x (n rounded up to 4): the thresholded point of every lockstep column
  DevBuf<double> nrm2;               // 16 x ngroups squared group norms
  void reset() { *this = FeatureGroups{}; }
};

// Scratch sized by the shape and the CU count alone: nothing invalidates it.  gbuf_own ... part: fos_problem_create; the rest
// on first use by the entry point named.
struct Scratch {
  DevBuf<float> gbuf_own;            // n + 4 floats
  DevBuf<float> ybuf;                // n floats: aligned copy of a caller vector when needed
  DevBuf<double> dscal;              // 256 device doubles (scalars)
  DevBuf<double> part;               // partial sums of the small kernels
  DevBuf<double> lhist;              // fos_power_iter: L after every step (n_iter + 1 doubles, grown on demand)
  DevBuf<float> vring;               // fos_power_iter, streaming plans: the iterates of the last 16 steps (16 x n rounded up to 4)
  DevBuf<float> rcols16;             // column-sharded candidate pass: m x 16 partial residuals (summed over the ranks)
  DevBuf<float> b16;                 // several right-hand sides: m x 16 zero-padded block of the caller's B (stage_b16)
  DevBuf<double> link_part;          // fos_residual_batch / _folds behind a link kernel: its partials of all panels (panels x ncu x 16; pointwise link: x 2 ncu); fos_multinomial_gradient_batch: the softmax link's likewise
  DevBuf<double> grad_part;          // fos_gradient_batch with loss16 on several row panels: product 1's partials of all panels (panels x (3 ncu + 8) x 16)
  DevBuf<double> dual_part;          // fos_duality_gap, fos_multinomial_duality_gap: the row pass's partials of all panels (panels x 2 ncu x 32)
  DevBuf<double> dual_col;           // fos_duality_gap, fos_multinomial_duality_gap: the column pass's 16 scales, 16 penalty sums and 16 conjugate sums
  DevBuf<double> mfold;              // column-sharded lockstep: 16 x 4 folded step partials (summed over the ranks)
  DevBuf<double> cr_part;            // chip-resident loop (chip_resident.hpp): [2][G][17] partials + [8] step sums + [1] rr
  DevBuf<unsigned> cr_bar;
  // fused persistent step (fused_step.hpp, fos_fista_run_fused): barrier words, per-workgroup partials, beta sequence
  DevBuf<unsigned> fz_bar;
  DevBuf<double> fz_part;
  DevBuf<double> fz_beta;            // also the chip-resident loop's; iters + 1 doubles, grown on demand
};

struct fos_problem {
  // the caller's: never freed here
  const void* A = nullptr;
  const float* b = nullptr;
  float* gbuf = nullptr;             // n + 4 floats: ws.gbuf_own, or the caller's after fos_problem_set_gbuf
  unsigned long long* fz_stamps = nullptr;   // fos_problem_set_fused_stamps, [ncu][8]
  fos_comm* comm = nullptr;          // row-sharded problem: sums of partial results go through it (comm.hpp)
  int64_t m = 0, n = 0, lda = 0;
  int dtype = FOS_F32;
  int loss = FOS_LOSS_SQUARED;       // fos_problem_set_loss / _set_multinomial: what b means to the matrix-core lockstep (no buffer depends on it)
  double link_param = 0.0;           // fos_problem_set_link_loss: the threshold c of a Huber problem; 0 otherwise
  int classes = 0;                   // fos_problem_set_multinomial: C of a multinomial problem (b holds class indices 0 .. C-1); 0 otherwise
  const float* row_weight = nullptr; // fos_row_weights_bind: the caller's m per-row weights of the data term (borrowed; nullptr: none)
  // fos_coord_bind: per-coordinate penalty factors and box bounds of the lockstep's update (borrowed; nullptr: 1, -inf, +inf)
  const float* coord_factor = nullptr;
  const float* coord_lo = nullptr;
  const float* coord_hi = nullptr;
  hipStream_t stream = nullptr;
  int ncu = 256;
  // inputs of the plan groups besides the shape (set by the entry point named; see fosapi::invalidate)
  bool col_sharded = false;          // comm splits the COLUMNS instead: this rank holds A[:, its columns], x is partitioned
  unsigned plan_flags = 0;           // FOS_PLAN_* given to fos_problem_replan
  bool allow_resident = true;
  bool il = false;                   // rows dealt round-robin to the workgroups (FOS_PLAN_INTERLEAVE / planner default for big rows)
  int dd_nwg_hint = 0;               // fos_problem_tune_dd: workgroups of the streaming fp64 pass (0 = planner)
  int cp_mode = 0;                   // 0: planner's choice, 1: FOS_PLAN_CLUSTER, 2: FOS_PLAN_NO_CLUSTER
  int chip_mode = 0;                 // 0: planner (fos_fista_run_chip where it measured ahead), 1: FOS_PLAN_CHIP_RESIDENT, 2: never
  int pack_mode = 0;                 // 0: planner (from the break-even size on), 1: FOS_PLAN_PACK, 2: FOS_PLAN_NO_PACK
  bool fused_on = false;             // FOS_PLAN_FUSED_MFMA: plain fos_fista_run calls take fos_fista_run_fused where served
  unsigned cp_epoch = 1;             // launch epoch of the one-read cluster pass
  // decisions and the workspace they size
  PassPlan pass;
  DdPlan dd;
  MultiPlan multi;
  DdMultiPlan dm;
  CandPlan cand;
  PackPlan pk;
  FeatureGroups fg;
  Scratch ws;
  std::unique_ptr<LbfgsWork> lbfgs;              // fos_lbfgs_minimize workspace, allocated by the first fit
  std::unique_ptr<LbfgsMultiWork> lbfgs_multi;   // fos_lbfgs_minimize_multi workspace
  // optional kernel timing (fos_problem_profile)
  int profiling = 0;                 // 0 off, N: bracket every N-th launch of the A pass
  int64_t prof_seq = 0;
  bool prof_open = false;
  std::vector<hipEvent_t> ev_pool;   // pairs: [2i] start, [2i+1] stop
  size_t ev_used = 0;
  double prof_ms = 0.0;
  int64_t prof_launches = 0;
};

// The momentum scalars t_k, beta_k and the count k live in FistaScalars on the device.  Plain runs (no adaptive restart, no
// stopping tolerance) follow a momentum sequence that does not depend on the data, so the host keeps a mirror of them and
// passes beta_k to the kernels by value; the scalar bookkeeping then runs once per call instead of once per iteration.
//   host_valid   h_t, h_beta, h_k are t_k, beta_k, k.  False once a run with data-dependent control (device-driven,
//                resident, controlled lockstep, non-plain split mode) has advanced the device scalars; the next plain run
//                reads them back once (one synchronisation).
//   pending      plain iterations have run whose bookkeeping (fista_finalize_plain_kernel) has not: the device scalars are
//                behind the mirror.  Every other entry point flushes first; a plain fos_fista_run closes them with its own
//                iterations.
//   plain_count  consecutive plain iterations whose step partials sit in part2 (slot k & 1); the closing bookkeeping reads the
//                previous step from part2 only when there are two.
//   y_valid      ynext holds y_{h_k} in fp32 (written by the previous update); otherwise the next pass forms y from x_k,
//                x_{k-1} and h_beta - bit-identical either way.
// fos_fista.hip assigns these fields only in its mirror helpers (begin_plain ... hand_to_device) and in create / reset.
struct fos_fista {
  fos_problem* p = nullptr;
  fos::FistaParams prm{};
  bool host_valid = false;
  double h_t = 1.0, h_beta = 0.0;
  long long h_k = 0;
  DevBuf<double> part2;              // ping-pong partials for plain runs: 2 * nupd * 4 doubles
  DevBuf<float> ynext;               // plain runs: y_{k+1} in fp32 written by the update kernel
  bool y_valid = false;
  bool pending = false;
  long long plain_count = 0;
  DevBuf<double> x_cur, x_prev;      // fp64 iterate state
  DevBuf<float> dlt;                 // trial difference vector x_tmp - y_k (fp32)
  DevBuf<fos::FistaScalars> scal;
  // precise mode (fos_fista_set_precise): the split-form gradient comes from the fp64-accumulating pass at the unrounded
  // fp64 y_k, so that the Armijo comparison g(x_tmp) <= g(y) + C grad.dlt is decided on fp64-accurate terms
  bool precise = false;
  DevBuf<double> folded;             // column-sharded: the 4 update sums of an iteration, folded and summed over the ranks
  bool tau_on_device = false;        // FistaScalars::tau is authoritative (device-driven backtracking ran since the last set_tau / reset)
  double* gbuf64 = nullptr;          // n + 4 doubles: [gradient ; ||r||^2] - gbuf64_own, or the caller's (fos_fista_set_gbuf64)
  DevBuf<double> gbuf64_own;         // allocated by fos_fista_set_precise when the caller gave none
  DevBuf<double> out5;
  int nupd = 0;                      // workgroups of the update kernel
};

namespace fosapi {

// ---- fos_plan.hip ---------------------------------------------------------------------------------------------------
const MenuEntry* wide_entry(int dtype);           // the y-in-LDS pass (gemv_wide.hpp): 16385..32768 fp32, 24577..32768 bf16 columns
const MenuEntry* find_entry(int dtype, int threads, int k, int r);
const MenuEntry* default_entry(int dtype, int64_t n);
int epc_of(int dtype);
int grid_1d(int64_t n, int per_block, int cap);
void plan_fused(fos_problem* p, const MenuEntry* e, int nwg_hint);
void apply_plan(fos_problem* p, unsigned flags);
// An input of the plan changed: reset every group derived from it (the groups and their inputs: fos_problem above).  Each
// group is rebuilt by its planner function on the next use.
enum PlanInput : unsigned {
  IN_PLAN = 1,       // plan flags, column sharding: the fp32 pass is planned anew
  IN_TUNE = 2,       // fos_problem_tune: the fp32 pass's geometry or grid
  IN_TUNE_DD = 4,    // fos_problem_tune_dd
  IN_COMM = 8,       // a communicator attached or detached
  IN_CLUSTER = 16,   // the runtime refused the one-read cluster launch: cp_mode is now "never"
};
int invalidate(fos_problem* p, unsigned changed);
// Layout of the matrix-core lockstep (run_multi_mfma), planned on first use: the one-read cluster form or two products per row
// panel; fills the MultiPlan group.
int plan_multi_mfma(fos_problem* p);
int ensure_workspace(fos_problem* p);
int ensure_batch_workspace(fos_problem* p);
int ensure_dd(fos_problem* p);
// Make the packed copy of A where the plan, the data and free memory allow (PackPlan); a refusal is not an error.  Synchronises.
int ensure_packed(fos_problem* p);
int prof_drain(fos_problem* p);
int prof_mark(fos_problem* p, bool start);
int aligned_vec(fos_problem* p, const float* v, const float** out);
bool batch_supported(const fos_problem* p);
MultiLaunch find_multi(int64_t n, int nv, bool bblock = false);
// the caller's X (n x 16 floats, columns 0..nv-1) -> p->cand.xp in the layout product 1 reads (after ensure_batch_workspace)
int pack_candidates(fos_problem* p, const float* X, int nv);
// several right-hand sides: the caller's B (m x nv, leading dimension ldb) -> p->b16, zero beyond column nv
int stage_b16(fos_problem* p, const float* B, int64_t ldb, int nv);
// Enqueue the A pass for `ys`.  with_g: also produce the slabs (A^T r).  *n_rr: number of rr partials written.
// rr_to (single-pass streaming plans only; the caller checks): the caller's nwg doubles that take the partials of ||A y - b||^2
// - of ||A x_k - b||^2 for a DUAL pass - instead of the handle's own.
int launch_pass(fos_problem* p, const YSource& ys, const float* b, bool with_g, int* n_rr, bool dual = false,
                double* rr_to = nullptr);
// slabs -> gbuf[0..n], summed over the ranks when the problem is row-sharded; rr_out (nullable) = the global ||r||^2
int launch_slab_reduce(fos_problem* p, int n_rr, float* gbuf, double* rr_out, const int* stopped);
// held (HOST, nv entries, each -1..254) -> the by-value block of the fold kernels, the slots beyond nv set to -1 (in either
// mode such a column is all zero: its candidate is).  False when an entry is out of range.
bool fold_held_block(const int32_t* held, int nv, fos::FoldHeld* out);
// What one launch of product 1 (batch_trial.hpp) can be given; a zero or null member is "off".  On `rows` rows starting at
// A / b / fold_of_row / row_weight: q_part[wg][16] takes the partial sums of every column, rout (nullable) the residual block R.
struct BatchLaunch {
  const void* A;                 // fp32 or bf16, as the problem's dtype says
  const float* b;                // subtracted when use_b is set (the labels of a logistic problem)
  int use_b;                     // 0: R = A Y, the squared form on any problem (fos_gram_apply, the line search)
  int64_t rows;
  float* rout;
  bool bblock;                   // b is the rows x 16 right-hand-side block: column j subtracts its own b[row * 16 + j]
  const int* stopped;            // device flag: the launch is a no-op while it is set
  const uint8_t* fold_of_row;    // the fold mask of K-fold cross-validation (with held; both or neither): with rout R is zero
  const fos::FoldHeld* held;     // on every column's held-out rows (FOLD_TRAIN), without rout the sums run over them (FOLD_HELD)
  const float* row_weight;       // R and the sums are weighted per row
};
// The one launcher of product 1: the form (STORE_R, BBLOCK, FOLD, LOSS, WEIGHT) follows from L and the problem's loss and is
// looked up in the one table of launchable forms (fos_plan.hip kBatchForms); *nwg_out = the rows of q_part written.
int launch_batch_product(fos_problem* p, const BatchLaunch& L, int* nwg_out);
// The link kernel of a multinomial problem (softmax_link.hpp) on the `rows` rows of p->multi.rbuf16 that product 1 has just
// filled with the logits of the panel starting at row0: R in place (not in the held-out form), q_part[wg][16] the loss sums of
// the segments; labels, weights and fold ids are offset by row0 here.  fold: FOLD_OFF / FOLD_TRAIN / FOLD_HELD (fold_of_row and
// held non-null unless FOLD_OFF).  *nwg_out = the rows of q_part written (at most p->ncu).
int launch_softmax_link(fos_problem* p, int64_t row0, int64_t rows, int nv, int fold, const uint8_t* fold_of_row,
                        const fos::FoldHeld* held, double* q_part, int* nwg_out);
// A problem with the Huber or the squared-hinge loss (fos_problem_set_link_loss): the pointwise link kernel sits between the
// two products.
inline bool link_loss(const fos_problem* p) { return p->loss == FOS_LOSS_HUBER || p->loss == FOS_LOSS_SQUARED_HINGE; }
// need_squared's refusal of such a problem, with a text of its own (FOS_OK on any other problem).
int link_refusal(const fos_problem* p, const char* fn);
// The link kernel of such a problem (pointwise_link.hpp), with the panel contract of launch_softmax_link: any nv in 1..16,
// *nwg_out = the rows of q_part written (at most 2 * p->ncu).
int launch_pointwise_link(fos_problem* p, int64_t row0, int64_t rows, int nv, int fold, const uint8_t* fold_of_row,
                          const fos::FoldHeld* held, double* q_part, int* nwg_out);
// Whether the nv columns split into whole class groups of a multinomial problem and (held non-null: HOST ids) every group
// holds out one fold.
bool softmax_groups_ok(const fos_problem* p, int nv, const int32_t* held);
// The one guard of the entry points that form an unweighted squared-loss residual, gradient or objective: refuses a logistic
// problem and a problem with row weights (FOS_ERR_UNSUPPORTED) before any launch or change of handle state.
int need_squared(const fos_problem* p, const char* fn);
// Coordinate data (fos_coord_bind) is served by the update of the two-product lockstep alone: has_coord says whether any of
// the three vectors is bound, coord_refusal is need_squared's third refusal (FOS_OK on a problem without coordinate data).
inline bool has_coord(const fos_problem* p) { return p->coord_factor || p->coord_lo || p->coord_hi; }
int coord_refusal(const fos_problem* p, const char* fn);
// Feature groups (fos_feature_groups_bind) likewise: has_fgroups says whether a table is bound, fgroup_refusal is need_squared's
// refusal of such a problem, in front of the coordinate one (FOS_OK on a problem without feature groups).
inline bool has_fgroups(const fos_problem* p) { return p->fg.ngroups > 0; }
int fgroup_refusal(const fos_problem* p, const char* fn);
// q[j] = ||A Xp_j - use_b*b||^2 -> out16 (device); Xp already in p->xp.  b16 (unsharded only): subtract its column j instead
int launch_residual_batch(fos_problem* p, int use_b, double* out16, const int* stopped = nullptr, const float* b16 = nullptr);
int launch_cluster_pass(fos_problem* p);
// the fp64-accumulating pass for any y source: out[0..n) = A^T (A y - b) + alpha2*l2vec, out[n] = ||A y - b||^2
int launch_pass_dd(fos_problem* p, const YSource& ys, double alpha2, const double* l2vec, double* out);
int gemv_pair_dd_stamped(fos_problem* p, const double* x, double alpha2, double* grad_rr, unsigned long long* t_stamp, bool* stamped);
int dd_pass_stamps(fos_problem* p, bool* yes);
// fp64 multi-point pass (gram_batch_dd.hpp) over the columns c.col[0..ncols) (bit j of `live`: column j takes part; the
// others are zero in the staged block): g_j = A^T (A x_j - b16_j) + alpha2 x_j, *rr_j = ||A x_j - b16_j||^2.  b16: the
// staged m x 16 block (stage_b16).  FOS_ERR_UNSUPPORTED where the shape has no matrix-core pair (pair_dd_multi_supported).
bool pair_dd_multi_supported(const fos_problem* p);
int pair_dd_multi(fos_problem* p, const fos::DdMultiCols& c, int ncols, unsigned live, double alpha2, const float* b16);
// ---- fos_comm.hip ---------------------------------------------------------------------------------------------------
// in-place sum over the ranks of a communicator on `st`: RCCL, or the one-shot full-mesh kernel (comm.hpp)
int comm_allreduce(fos_comm* c, void* buf, size_t count, bool f64, hipStream_t st);
// sum `count` floats / doubles over the ranks of a sharded problem, in place, on the handle's stream (no-op otherwise)
int reduce_across(fos_problem* p, void* buf, size_t count, bool f64);

// ---- batches of small problems (fos_fista_run_batch, fos_power_iter_batch) -------------------------------------------
// The descriptor checks both entry points make before any HIP call: FOS_ERR_ARG for a negative offset, lda < n or n > ld
// (ld: the caller's stride of the per-problem n-vectors), FOS_ERR_UNSUPPORTED outside the LDS-resident limits.
inline int check_batch_items(const char* fn, const fos_batch_item* items, int count, int64_t ld) {
  for (int i = 0; i < count; ++i) {
    const fos_batch_item& it = items[i];
    if (it.a_offset < 0 || it.b_offset < 0 || it.n < 1 || it.m < 1 || it.lda < it.n || it.n > ld)
      return fail(FOS_ERR_ARG, std::string(fn) + ": bad argument (item " + std::to_string(i) +
                                   ": negative offset, empty shape, lda < n or n > the vector stride)");
    if (!fos::resident_fits(it.m, it.n))
      return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": item " + std::to_string(i) +
                                           " does not fit the LDS-resident loop (n <= 64, m <= 4096, m * (n | 1) <= 10240)");
  }
  return FOS_OK;
}

}  // namespace fosapi
