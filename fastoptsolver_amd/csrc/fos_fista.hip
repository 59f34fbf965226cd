// libfos_hip.so, translation unit 3 of 4 - the FISTA / ISTA / FISTA-delta state machine of the C ABI (include/fos.h):
// fused, split, recorded, backtracking, resident and lockstep (multi-lambda) runs.  iterative_solvers.py:65-344.
#include "fos_internal.hpp"
#include "fused_step.hpp"
#include "chip_resident.hpp"
#include "working_set.hpp"
#include "duality.hpp"
#include "multinomial_ws.hpp"
#include "resample_link.hpp"
#include <cassert>

using namespace fosapi;

template <int NQ>
static int launch_fused(const fos::FusedArgs& a, int G, size_t lds, hipStream_t st) {
  auto kern = fos::fista_fused_kernel<NQ>;
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const uint64_t bit = 1ull << (dev & 63);
  if (!(done.load(std::memory_order_acquire) & bit)) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    done.fetch_or(bit, std::memory_order_release);
  }
  // a plain launch: G = #CUs workgroups of 512 threads and ~136 KiB of LDS are co-resident by grid size (one per CU), which
  // is all hipLaunchCooperativeKernel would check; every grid-wide wait in the kernel is bounded
  hipLaunchKernelGGL(kern, dim3(G), dim3(fos::FZ_THREADS), lds, st, a);
  LAUNCH_CHECK();
  return FOS_OK;
}

template <int NC, bool CTRL>
static int launch_chip(const fos::ChipArgs& a, int G, size_t lds, hipStream_t st) {
  auto kern = fos::fista_chip_resident_kernel<NC, CTRL>;
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const uint64_t bit = 1ull << (dev & 63);
  if (!(done.load(std::memory_order_acquire) & bit)) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, fos::CR_LDS_BUDGET));
    done.fetch_or(bit, std::memory_order_release);
  }
  // a plain launch of at most #CUs workgroups with up to 150 KiB of LDS each: co-resident by grid size; every wait is bounded
  hipLaunchKernelGGL(kern, dim3(G), dim3(fos::CR_THREADS), lds, st, a);
  LAUNCH_CHECK();
  return FOS_OK;
}

extern "C" {

// ---- FISTA ---------------------------------------------------------------------------------------------
int fos_fista_create(fos_problem* p, fos_fista** out) {
  if (!p || !out) return fail(FOS_ERR_ARG, "fos_fista_create: null");
  fos_fista* f = new fos_fista();
  f->p = p;
  f->nupd = (int)((p->n + fos::RCOLS - 1) / fos::RCOLS);
  int rc;
  if ((rc = f->x_cur.reserve(p->n)) || (rc = f->x_prev.reserve(p->n)) || (rc = f->dlt.reserve(p->n)) || (rc = f->scal.reserve(1)) ||
      (rc = f->out5.reserve(8)) || (rc = f->part2.reserve((size_t)2 * f->nupd * 4)) || (rc = f->ynext.reserve(p->n))) {
    delete f;
    return rc;
  }
  *out = f;
  return FOS_OK;
}

int fos_fista_destroy(fos_fista* f) {
  delete f;
  return FOS_OK;
}

static void to_dev_params(const fos_fista_params* s, fos::FistaParams* d) {
  d->alpha1 = s->alpha1;
  d->alpha2 = s->alpha2;
  d->tau = s->tau;
  d->mode = s->mode;
  d->prox_kind = s->prox_kind;
  d->delta = s->delta;
  d->adaptive_restart = s->adaptive_restart;
  d->restart_threshold = s->restart_threshold;
  d->tol_step = s->tol_step;
  d->tol_ratio = s->tol_ratio;
  d->tol_grad = s->tol_grad;
  d->tau_from_state = 0;
  d->group = s->group;
}

int fos_fista_reset(fos_fista* f, const fos_fista_params* prm, const double* x0) {
  if (!f || !prm) return fail(FOS_ERR_ARG, "fos_fista_reset: null");
  if (prm->mode < 0 || prm->mode > 2 || prm->prox_kind < 0 || prm->prox_kind > 1 || !(prm->tau > 0.0) ||
      prm->tol_grad < 0.0 || prm->tol_step < 0.0 || prm->tol_ratio < 0.0)
    return fail(FOS_ERR_ARG, "fos_fista_reset: bad mode/prox_kind/tau/tolerance");
  if (prm->group < 0 || prm->group > fos::BT_NV)
    return fail(FOS_ERR_ARG, "fos_fista_reset: group outside 0..16 (the columns of one group penalty)");
  to_dev_params(prm, &f->prm);
  fos_problem* p = f->p;
  const size_t nb = (size_t)p->n * sizeof(double);
  if (x0) {
    HIP_TRY(hipMemcpyAsync(f->x_cur, x0, nb, hipMemcpyDeviceToDevice, p->stream));
    HIP_TRY(hipMemcpyAsync(f->x_prev, x0, nb, hipMemcpyDeviceToDevice, p->stream));
  } else {
    HIP_TRY(hipMemsetAsync(f->x_cur, 0, nb, p->stream));
    HIP_TRY(hipMemsetAsync(f->x_prev, 0, nb, p->stream));
  }
  hipLaunchKernelGGL(fos::fista_init_scalars_kernel, dim3(1), dim3(1), 0, p->stream, f->scal);
  LAUNCH_CHECK();
  f->host_valid = true;
  f->tau_on_device = false;
  f->y_valid = false;
  f->pending = false;
  f->plain_count = 0;
  f->h_t = 1.0;
  f->h_beta = 0.0;
  f->h_k = 0;
  return FOS_OK;
}

int fos_fista_set_tau(fos_fista* f, double tau) {
  if (!f || !(tau > 0.0)) return fail(FOS_ERR_ARG, "fos_fista_set_tau: bad argument");
  f->prm.tau = tau;
  f->tau_on_device = false;
  return FOS_OK;
}

// The one guard of the entry points that advance or evaluate a single state machine: a handle under the group penalty
// (fos_fista_params.group >= 2) is one column of a joint fit and its prox needs the other columns, so none of them may answer
// for it with the separable prox.  Refuses before any launch or change of handle state; the lockstep entry points serve it.
static bool grouped(const fos::FistaParams& prm) { return prm.group >= 2; }
static int need_separable(const fos_fista* f, const char* fn) {
  if (f && grouped(f->prm))
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": not served on a handle under the group penalty (fos_fista_params.group >= 2); "
                                     "it runs through fos_fista_run_multi / _run_multi_rhs / _run_multi_folds");
  return FOS_OK;
}

static fos::GradSrc grad_src(const fos_fista* f) {
  return fos::GradSrc{f->p->gbuf, f->precise ? f->gbuf64 : nullptr};
}

int fos_fista_set_precise(fos_fista* f, int on) {
  if (!f) return fail(FOS_ERR_ARG, "fos_fista_set_precise: null");
  if (on && !f->gbuf64) {
    if (int rc = f->gbuf64_own.reserve(f->p->n + 4)) return rc;
    f->gbuf64 = f->gbuf64_own;
  }
  f->precise = on != 0;
  return FOS_OK;
}

int fos_fista_set_gbuf64(fos_fista* f, double* buf) {
  if (!f) return fail(FOS_ERR_ARG, "fos_fista_set_gbuf64: null");
  if (buf && (reinterpret_cast<uintptr_t>(buf) & 15u)) return fail(FOS_ERR_ARG, "fos_fista_set_gbuf64: misaligned");
  f->gbuf64_own.reset();
  f->gbuf64 = buf;
  if (!buf) f->precise = false;
  return FOS_OK;
}

__global__ void rr_from_gbuf64_kernel(const double* __restrict__ g64, int n, double* __restrict__ rr_out, const int* stopped) {
  if (stopped != nullptr && *stopped != 0) return;
  *rr_out = g64[n];
}

static YSource fista_source(fos_fista* f) {
  return YSource{nullptr, f->x_cur, f->x_prev, &f->scal->beta, &f->scal->stopped, 0.0};
}

__global__ __launch_bounds__(64) void fold4_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out4,
                                                   const int* stopped) {
  if (stopped != nullptr && *stopped != 0) return;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += 64)
    for (int j = 0; j < 4; ++j) s[j] += part[i * 4 + j];
  for (int j = 0; j < 4; ++j) s[j] = fos::wave_sum(s[j]);
  if (threadIdx.x == 0)
    for (int j = 0; j < 4; ++j) out4[j] = s[j];
}

// Column-sharded lockstep: the step partials of every weight folded to [weight][4] (re-derived every iteration - the
// in-place all-reduce behind it must never see its own result, stopped weights included).
__global__ __launch_bounds__(64) void fold4_multi_kernel(fos::MultiControl mc, int nparts, double* __restrict__ out) {
  const int v = blockIdx.x;
  const double* part = mc.part[v];
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += 64)
    for (int j = 0; j < 4; ++j) s[j] += part[i * 4 + j];
  for (int j = 0; j < 4; ++j) s[j] = fos::wave_sum(s[j]);
  if (threadIdx.x == 0)
    for (int j = 0; j < 4; ++j) out[v * 4 + j] = s[j];
}

static int launch_finalize(fos_fista* f, int n_rr, double* hist_row = nullptr) {
  fos_problem* p = f->p;
  const double* part = p->ws.part;
  int nparts = f->nupd;
  if (p->col_sharded) {
    // x is partitioned over the ranks: step norms, ||grad||^2, ||x||_1, ||x||^2 are sums over ALL column blocks
    if (int rc = f->folded.reserve(8)) return rc;
    hipLaunchKernelGGL(fold4_kernel, dim3(1), dim3(64), 0, p->stream, p->ws.part, f->nupd, f->folded, (const int*)nullptr);   // re-derived after a stop: the in-place all-reduce below must never see its own result
    LAUNCH_CHECK();
    int rc = reduce_across(p, f->folded, 4, true);
    if (rc) return rc;
    part = f->folded;
    nparts = 1;
  }
  hipLaunchKernelGGL(fos::fista_finalize_kernel, dim3(1), dim3(64), 0, p->stream, part, nparts, p->pass.rr_part, n_rr,
                     f->scal, f->prm, hist_row);
  LAUNCH_CHECK();
  return FOS_OK;
}

// Momentum of the iteration that follows iteration index k (0-based), given t_k: iterative_solvers.py:215-216, :330.
static void host_momentum(const fos::FistaParams& prm, long long k, double* t, double* beta) {
  if (prm.mode == fos::MODE_FISTA) {
    const double t_new = 0.5 * (1.0 + std::sqrt(1.0 + 4.0 * (*t) * (*t)));
    *beta = (*t - 1.0) / t_new;
    *t = t_new;
  } else if (prm.mode == fos::MODE_DELTA) {
    const double kk = (double)(k + 1);
    *beta = kk / (kk + 1.0 + prm.delta);
  } else {
    *beta = 0.0;
  }
}

// fista_update_kernel: the gradient from the slab sets (slabs != null) or from gsrc; vec4: float4 epilogues
static int launch_update(fos_fista* f, const float* slabs, int nslabs, fos::GradSrc gsrc, const fos::FistaParams& prm,
                         double* part, int host_beta, double beta_val, double* x_hist, float* y_next, double beta_next,
                         int64_t slab_stride = 0, int y_mode = fos::YOUT_VECTOR, int y_slot = 0) {
  fos_problem* p = f->p;
#define FOS_UPDATE(FROM_SLABS, VEC)                                                                                             \
  hipLaunchKernelGGL((fos::fista_update_kernel<FROM_SLABS, VEC>), dim3(f->nupd), dim3(256), 0, p->stream, slabs, nslabs, gsrc,  \
                     (int)p->n, f->x_cur, f->x_prev, f->scal, prm, part, host_beta, beta_val, x_hist, y_next, beta_next,       \
                     slab_stride, y_mode, y_slot)
  if (slabs) { if (p->pass.vec4) FOS_UPDATE(true, true); else FOS_UPDATE(true, false); }
  else { if (p->pass.vec4) FOS_UPDATE(false, true); else FOS_UPDATE(false, false); }
#undef FOS_UPDATE
  LAUNCH_CHECK();
  return FOS_OK;
}

static int launch_update_from_slabs(fos_fista* f, double* part, int host_beta, double beta_val,
                                    double* x_hist = nullptr, float* y_next = nullptr, double beta_next = 0.0,
                                    const float* slabs = nullptr, int64_t slab_stride = 0, int nslabs = 0,
                                    int y_mode = fos::YOUT_VECTOR, int y_slot = 0) {
  fos_problem* p = f->p;
  return launch_update(f, slabs ? slabs : p->pass.slabs, nslabs ? nslabs : p->pass.nslabs, fos::GradSrc{nullptr, nullptr}, f->prm, part,
                       host_beta, beta_val, x_hist, y_next, beta_next, slab_stride ? slab_stride : p->pass.slab_stride, y_mode, y_slot);
}

// y source of a plain-run iteration: the fp32 vector the previous update kernel wrote, or the fp64 state with the host's beta
static YSource plain_source(fos_fista* f) {
  if (f->y_valid) return YSource{f->ynext, nullptr, nullptr, nullptr, &f->scal->stopped, 0.0, nullptr};
  return YSource{nullptr, f->x_cur, f->x_prev, nullptr, &f->scal->stopped, f->h_beta, nullptr};
}

// ---- The host mirror of the momentum scalars (struct fos_fista, fos_internal.hpp): its only writers ----------------------
static double* part2_slot(const fos_fista* f, long long k) { return f->part2 + (size_t)(k & 1) * f->nupd * 4; }

// The closing fista_finalize_plain_kernel of plain iterations: step partials (nparts x 4) of the last iteration (cur) and of
// the one before it (prev; null: none), rr partials (n_rr = 0: rr was written already), momentum and count from the mirror.
static int finish_plain(fos_fista* f, const double* cur, const double* prev, int nparts, const double* rr, int n_rr) {
  hipLaunchKernelGGL(fos::fista_finalize_plain_kernel, dim3(1), dim3(64), 0, f->p->stream, cur, prev, nparts, rr, n_rr, f->scal,
                     f->h_t, f->h_beta, f->h_k);
  LAUNCH_CHECK();
  f->pending = false;
  return FOS_OK;
}

// ... of plain iterations whose partials sit in part2
static int finish_part2(fos_fista* f, int n_rr) {
  return finish_plain(f, part2_slot(f, f->h_k - 1), f->plain_count >= 2 ? part2_slot(f, f->h_k - 2) : nullptr, f->nupd,
                      f->p->pass.rr_part, n_rr);
}

static int flush_pending(fos_fista* f) { return f->pending ? finish_part2(f, 0) : FOS_OK; }

// Start of a plain run: flush (unless the run closes the pending iterations itself), then the mirror valid - read back once
// after device-held state.  *stopped: the state machine has stopped; the caller decides what that means for its run.  The
// mirror of a stopped state stays invalid, so every later plain call asks again: a valid mirror says "not stopped".
static int begin_plain(fos_fista* f, bool* stopped, bool flush = true) {
  *stopped = false;
  int rc = flush ? flush_pending(f) : FOS_OK;
  if (rc || f->host_valid) return rc;
  fos_fista_status st;
  if ((rc = fos_fista_status_get(f, &st))) return rc;
  *stopped = st.stopped != FOS_STOP_NONE;
  if (*stopped) return FOS_OK;
  f->h_t = st.t_prev; f->h_beta = st.beta; f->h_k = st.k;
  f->host_valid = true;
  return FOS_OK;
}

// One plain iteration k = h_k: beta_k of its y, beta_{k+1} of the next y, its part2 slot.  ynext: its update leaves y_{k+1}
// there.
struct PlainStep { double beta, beta_next; double* part; };
static PlainStep advance_plain(fos_fista* f, bool ynext) {
  PlainStep s{f->h_beta, 0.0, part2_slot(f, f->h_k)};
  host_momentum(f->prm, f->h_k, &f->h_t, &f->h_beta);
  s.beta_next = f->h_beta;
  f->h_k += 1;
  f->plain_count += 1;
  f->y_valid = ynext;
  f->pending = true;
  return s;
}

// The momentum of `iters` plain iterations run in one launch: beta_k for y_k, then beta_{k+1} ... beta_{k+iters} -> p->ws.fz_beta.
// The mirror moves on by iters; *before is where it stood (restore_momentum).
struct Momentum { double t, beta; long long k; };
static int momentum_sequence(fos_fista* f, int iters, Momentum* before) {
  fos_problem* p = f->p;
  if (int rc = p->ws.fz_beta.reserve((size_t)iters + 1)) return rc;
  *before = Momentum{f->h_t, f->h_beta, f->h_k};
  std::vector<double> betas((size_t)iters + 1);
  betas[0] = f->h_beta;
  for (int k = 0; k < iters; ++k) {
    host_momentum(f->prm, f->h_k, &f->h_t, &f->h_beta);
    betas[(size_t)k + 1] = f->h_beta;
    f->h_k += 1;
  }
  HIP_TRY(hipMemcpyAsync(p->ws.fz_beta, betas.data(), betas.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));          // (the host vector must outlive the copy)
  return FOS_OK;
}

static void restore_momentum(fos_fista* f, const Momentum& m) {
  f->h_t = m.t; f->h_beta = m.beta; f->h_k = m.k;
}

// ynext must hold y_{h_k}
static int ensure_y(fos_fista* f) {
  if (f->y_valid) return FOS_OK;
  fos_problem* p = f->p;
  hipLaunchKernelGGL(fos::form_y_kernel, dim3(grid_1d(p->n, 256, 256)), dim3(256), 0, p->stream, f->x_cur, f->x_prev, f->h_beta,
                     f->ynext, p->n);
  LAUNCH_CHECK();
  f->y_valid = true;
  return FOS_OK;
}

// The next plain iteration starts a new run of part2 partials, and forms its y from the fp64 state unless keep_y.
static void restart_plain(fos_fista* f, bool keep_y = false) {
  f->plain_count = 0;
  if (!keep_y) f->y_valid = false;
}

// t, beta and k advance on the device only from here on
static void hand_to_device(fos_fista* f) {
  f->host_valid = false;
  restart_plain(f);
}

static bool plain_run(const fos_fista* f) {
  return !(f->prm.mode == fos::MODE_FISTA && f->prm.adaptive_restart) && f->prm.tol_step == 0.0 &&
         f->prm.tol_ratio == 0.0 && f->prm.tol_grad == 0.0;
}

// The gradient-norm stop sits between the reduced gradient and the update (fos_fista_params.tol_grad).
static int launch_grad_norm_stop(fos_fista* f) {
  fos_problem* p = f->p;
  if (p->col_sharded) {                        // ||grad||^2 = sum over the column blocks of all ranks
    if (int rc = f->folded.reserve(8)) return rc;
    hipLaunchKernelGGL(fos::grad_norm_stop_kernel, dim3(1), dim3(1024), 0, p->stream, grad_src(f), (int)p->n, f->x_cur,
                       f->x_prev, f->scal, f->prm, f->folded + 4);
    LAUNCH_CHECK();
    int rc = reduce_across(p, f->folded + 4, 1, true);
    if (rc) return rc;
    hipLaunchKernelGGL(fos::grad_norm_decide_kernel, dim3(1), dim3(1), 0, p->stream, f->folded + 4, f->scal, f->prm);
    LAUNCH_CHECK();
    return FOS_OK;
  }
  hipLaunchKernelGGL(fos::grad_norm_stop_kernel, dim3(1), dim3(1024), 0, p->stream, grad_src(f), (int)p->n, f->x_cur, f->x_prev,
                     f->scal, f->prm);
  LAUNCH_CHECK();
  return FOS_OK;
}

// Whole run in ONE launch of ONE workgroup (resident.hpp): A, b and the iterate state stay in LDS.
static int run_resident(fos_fista* f, int iters, double* x_hist, double* hist, fos::ResidentOpts opt = fos::ResidentOpts{}) {
  fos_problem* p = f->p;
  if (opt.grad_tol == 0.0) opt.grad_tol = f->prm.tol_grad;     // the handle's own gradient-norm stop (:179)
  int rc = flush_pending(f);                   // device scalars must be current: the kernel continues from them
  if (rc) return rc;
  const bool small = p->n <= fos::RS_CHUNK && p->m <= fos::RS_SMALL_M;    // rows of A in registers (resident.hpp)
#define FOS_RS_LAUNCH(T, SMALL)                                                                                          \
  hipLaunchKernelGGL((fos::fista_resident_kernel<T, SMALL>), dim3(1), dim3(fos::RS_THREADS), 0, p->stream,               \
                     (const T*)p->A, p->lda, p->b, (int)p->m, (int)p->n, f->x_cur, f->x_prev, f->scal, f->prm, iters,    \
                     x_hist, hist, opt)
  if (p->dtype == FOS_F32) { if (small) FOS_RS_LAUNCH(float, true); else FOS_RS_LAUNCH(float, false); }
  else { if (small) FOS_RS_LAUNCH(fos::bf16_t, true); else FOS_RS_LAUNCH(fos::bf16_t, false); }
#undef FOS_RS_LAUNCH
  LAUNCH_CHECK();
  hand_to_device(f);
  return FOS_OK;
}

int fos_fista_run_resident(fos_fista* f, int iters, int backtracking, double eta, double armijo_c, double grad_tol,
                           double* x_hist, double* hist, int32_t* ls_iters, double* tau_hist, int32_t* iters_done,
                           double* tau_out) {
  if (!f || iters < 0 || !iters_done || !tau_out || (backtracking && !(eta > 0.0 && eta < 1.0)))
    return fail(FOS_ERR_ARG, "fos_fista_run_resident: bad argument");
  if (int rc_ = need_squared(f->p, "fos_fista_run_resident")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_run_resident")) return rc_;
  fos_problem* p = f->p;
  if (!p->pass.resident) return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_resident: problem does not fit the LDS-resident loop");
  *iters_done = 0;
  *tau_out = f->prm.tau;
  if (iters == 0) return FOS_OK;
  double* tau_dev = p->ws.dscal + 241;
  int* done_dev = reinterpret_cast<int*>(p->ws.dscal + 242);
  fos::ResidentOpts opt{backtracking ? 1 : 0, eta, armijo_c, grad_tol, ls_iters, tau_hist, tau_dev, done_dev};
  int rc = run_resident(f, iters, x_hist, hist, opt);
  if (rc) return rc;
  int done = 0;
  double tau = f->prm.tau;
  HIP_TRY(hipMemcpyAsync(&done, done_dev, sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipMemcpyAsync(&tau, tau_dev, sizeof(double), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  f->prm.tau = tau;                            // tau persists (iterative_solvers.py:197)
  *iters_done = done;
  *tau_out = tau;
  return FOS_OK;
}

int64_t fos_fista_history_workspace(fos_fista* f, int iters) {
  if (!f || iters < 0) return -1;
  return ((int64_t)(iters + 1) * f->p->pass.nwg + (int64_t)iters * f->nupd * 4) * (int64_t)sizeof(double);
}

int fos_fista_run_history(fos_fista* f, int iters, double* x_hist, double* hist, void* work) {
  if (!f || iters < 0 || (iters > 0 && (!x_hist || !hist || !work)))
    return fail(FOS_ERR_ARG, "fos_fista_run_history: bad argument");
  if (int rc_ = need_squared(f->p, "fos_fista_run_history")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_run_history")) return rc_;
  fos_problem* p = f->p;
  if (plain_run(f) && p->pass.resident) return iters == 0 ? FOS_OK : run_resident(f, iters, x_hist, hist);
  if (!plain_run(f) || p->pass.path != 0 || p->pass.colblock || p->pass.entry->dual == nullptr || p->comm != nullptr)
    return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_history: needs a plain run on the fused path with a DUAL kernel");
  if (iters == 0) return FOS_OK;
  bool stopped = false;
  int rc = begin_plain(f, &stopped);
  if (rc) return rc;
  if (stopped) return fail(FOS_ERR_STATE, "fos_fista_run_history: solver already stopped");
  const int nwg = p->pass.nwg;
  const size_t psz = (size_t)f->nupd * 4;
  double* rr2_slots = reinterpret_cast<double*>(work);                 // (iters + 1) x nwg
  double* part_slots = rr2_slots + (size_t)(iters + 1) * nwg;          // iters x nupd x 4
  int n_rr = 0;
  for (int it = 0; it < iters; ++it) {
    // the DUAL pass needs x_k itself, so it always forms y from the fp64 state
    YSource ys{nullptr, f->x_cur, f->x_prev, nullptr, &f->scal->stopped, f->h_beta, nullptr};
    // slot it = residual of the iterate BEFORE it
    if ((rc = launch_pass(p, ys, p->b, true, &n_rr, true, rr2_slots + (size_t)it * nwg))) return rc;
    const PlainStep s = advance_plain(f, false);
    if ((rc = launch_update_from_slabs(f, part_slots + it * psz, 1, s.beta, x_hist + (size_t)it * p->n))) return rc;
  }
  // closing residual pass: ||A x_last - b||^2 -> slot iters (written by the residual-only kernel into rr_part)
  hipLaunchKernelGGL(fos::cast_f64_f32_kernel, dim3(grid_1d(p->n, 256, 1024)), dim3(256), 0, p->stream, f->x_cur, p->ws.ybuf,
                     p->n);
  LAUNCH_CHECK();
  {
    YSource ys{p->ws.ybuf, nullptr, nullptr, nullptr, nullptr};
    if ((rc = launch_pass(p, ys, p->b, false, &n_rr, false, rr2_slots + (size_t)iters * nwg))) return rc;
  }
  hipLaunchKernelGGL(fos::history_fold_kernel, dim3(iters), dim3(64), 0, p->stream, rr2_slots, nwg, part_slots, f->nupd,
                     hist);
  LAUNCH_CHECK();
  rc = finish_plain(f, part_slots + (iters - 1) * psz, iters >= 2 ? part_slots + (iters - 2) * psz : nullptr, f->nupd,
                    p->pass.rr_part, nwg);
  restart_plain(f);
  return rc;
}

int fos_fista_run(fos_fista* f, int iters) {
  if (!f || iters < 0) return fail(FOS_ERR_ARG, "fos_fista_run: bad argument");
  if (int rc_ = need_squared(f->p, "fos_fista_run")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_run")) return rc_;
  fos_problem* p = f->p;
  if (iters == 0) return FOS_OK;
  if (int rc_ = ensure_packed(p)) return rc_;      // first run of a plan: the 28-bit copy of A, where it is served
  if (p->pass.resident) return run_resident(f, iters, nullptr, nullptr);
  // Tall-skinny runs without backtracking / history: A in the LDS of up to all CUs, one grid barrier per iteration
  // (chip_resident.hpp); adaptive restart and the step / ratio stops are decided on the device by every workgroup alike.  The
  // planner's own region is where the plain loop measured at least 1.4x ahead of the two launches below (tools/bench_chip.py:
  // 9000 ... 100000 x 5 5.6-7.7 us per iteration against 10.8-11.2; runs with restart save a third launch on top);
  // FOS_PLAN_CHIP_RESIDENT / FOS_PLAN_NO_CHIP_RESIDENT widen it to every served shape / switch it off.
  {
    // (9..16 columns - the 16-column instantiation carries twice the registers: 20000 x 16 1.2x plain, 1.6x with restart, even at
    //  100000 x 16)
    const bool chip_region = p->dtype == FOS_F32 && p->m >= 512 && iters >= 8 &&
                             (p->n <= 8 ? p->m <= 131072 : (p->n <= 16 && p->m <= 32768));
    if ((p->chip_mode == 1 || (p->chip_mode == 0 && chip_region)) && !p->comm && !f->precise && !f->prm.tau_from_state &&
        f->prm.tol_grad == 0.0) {
      const int rcc = fos_fista_run_chip(f, iters);
      // not served, or its grid could not become co-resident within the bound (state untouched): the loops below
      if (rcc != FOS_ERR_UNSUPPORTED && rcc != FOS_ERR_STATE) return rcc;
    }
  }
  if (f->prm.tol_grad > 0.0 && !p->comm) {
    // gradient-norm stop: K2 -> slab reduce (gbuf) -> norm check -> update from gbuf -> finalize, all enqueued
    for (int it = 0; it < iters; ++it) {
      int rc;
      if ((rc = fos_fista_grad(f))) return rc;
      if ((rc = launch_grad_norm_stop(f))) return rc;
      if ((rc = fos_fista_update(f))) return rc;
    }
    return FOS_OK;
  }
  if (p->comm) {
    // Row-sharded problem: K2 on this rank's rows -> slab reduction -> all-reduce of [gradient ; ||r||^2] (n + 1 floats)
    // -> prox + momentum from the reduced gradient, all enqueued on one stream; every rank applies the identical fp64
    // update to identical numbers, so the replicated iterates stay bit-identical.
    for (int it = 0; it < iters; ++it) {
      int rc;
      if ((rc = fos_fista_grad(f))) return rc;
      if (f->prm.tol_grad > 0.0 && (rc = launch_grad_norm_stop(f))) return rc;
      if ((rc = fos_fista_update(f))) return rc;
    }
    return flush_pending(f);
  }
  // Plain run: no data-dependent control (adaptive restart / stopping tolerances).  t_k and beta_k are then a fixed
  // sequence: the host passes beta_k to both kernels by value, and the scalar bookkeeping kernel runs once per call
  // instead of once per iteration (two launches per iteration instead of three).
  if (plain_run(f) && p->fused_on && !f->precise && !f->prm.tau_from_state) {      // opt-in: the one-launch persistent step
    const int rcf = fos_fista_run_fused(f, iters);
    if (rcf != FOS_ERR_UNSUPPORTED) return rcf;
  }
  if (plain_run(f)) {
    bool stopped = false;
    int rc = begin_plain(f, &stopped, false);   // pending split-mode iterations close with this run's bookkeeping
    if (rc || stopped) return rc;
    int n_rr = 0;
    for (int it = 0; it < iters; ++it) {
      if ((rc = launch_pass(p, plain_source(f), p->b, true, &n_rr))) return rc;
      const PlainStep s = advance_plain(f, true);
      if ((rc = launch_update_from_slabs(f, s.part, 1, s.beta, nullptr, f->ynext, s.beta_next))) return rc;
    }
    return finish_part2(f, n_rr);
  }
  hand_to_device(f);
  for (int it = 0; it < iters; ++it) {
    int n_rr = 0, rc;
    if ((rc = launch_pass(p, fista_source(f), p->b, true, &n_rr))) return rc;
    if ((rc = launch_update_from_slabs(f, p->ws.part, 0, 0.0))) return rc;
    if ((rc = launch_finalize(f, n_rr))) return rc;
  }
  return FOS_OK;
}

// The step in ONE persistent launch with the row dots on the matrix cores and A staged through LDS (fused_step.hpp):
int fos_problem_set_fused_stamps(fos_problem* p, unsigned long long* stamps) {
  if (!p) return fail(FOS_ERR_ARG, "fos_problem_set_fused_stamps: null");
  p->fz_stamps = stamps;
  return FOS_OK;
}

// BASELINE north_star's literal design, opt-in (the two-launch VALU step measures faster).  Plain runs only.
int fos_fista_run_fused(fos_fista* f, int iters) {
  if (!f || iters < 0) return fail(FOS_ERR_ARG, "fos_fista_run_fused: bad argument");
  if (int rc_ = need_squared(f->p, "fos_fista_run_fused")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_run_fused")) return rc_;
  fos_problem* p = f->p;
  const int G = p->ncu;
  if (p->dtype != FOS_F32 || p->pass.path != 0 || p->pass.tall || p->pass.colblock || p->pass.resident || p->comm || p->n % 2048 != 0 ||
      p->n > 8192 || p->lda % 4 != 0 || (reinterpret_cast<uintptr_t>(p->A) & 15u) || p->m < 8 * (int64_t)G ||
      (p->n + G - 1) / G > fos::FZ_OWN_MAX)
    return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_fused: fp32 A, n in {2048, 4096, 6144, 8192}, aligned rows, m >= 8 x CUs, unsharded");
  if (!plain_run(f) || f->precise || f->prm.tau_from_state)
    return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_fused: plain runs only (no adaptive restart, tolerances, device-held step)");
  if (iters == 0) return FOS_OK;
  bool stopped = false;
  int rc = begin_plain(f, &stopped);
  if (rc || stopped) return rc;
  // workspace: G slabs (the planner's are reused when it planned G workgroups), barrier words, beta sequence, partials
  if ((rc = p->pass.slabs.reserve((size_t)G * p->n)) || (rc = p->pass.rr_part.reserve(G)) || (rc = p->pass.rr2_part.reserve(G)))
    return rc;
  if (!p->ws.fz_part) {
    if ((rc = p->ws.fz_bar.reserve(fos::FZ_BAR_WORDS))) return rc;
    HIP_TRY(hipMemsetAsync(p->ws.fz_bar, 0, fos::FZ_BAR_WORDS * sizeof(unsigned), p->stream));
    if ((rc = p->ws.fz_part.reserve((size_t)2 * G * 4))) return rc;
  }
  if ((rc = ensure_y(f))) return rc;
  Momentum before;
  if ((rc = momentum_sequence(f, iters, &before))) return rc;
  fos::FusedArgs a{};
  a.A = (const float*)p->A; a.lda = p->lda; a.b = p->b; a.m = p->m; a.n = (int)p->n;
  a.rows_per_wg = ((p->m + G - 1) / G + fos::FZ_ROWS - 1) / fos::FZ_ROWS * fos::FZ_ROWS;
  a.slabs = p->pass.slabs; a.y = f->ynext; a.x_cur = f->x_cur; a.x_prev = f->x_prev; a.beta = p->ws.fz_beta; a.part = p->ws.fz_part;
  a.rr_part = p->pass.rr_part; a.bar = p->ws.fz_bar; a.iters = iters; a.prox_kind = f->prm.prox_kind; a.k0 = before.k;
  a.tau = f->prm.tau; a.alpha1 = f->prm.alpha1; a.alpha2 = f->prm.alpha2;
  a.timeout_ticks = 100000000ull * 2ull;           // 2 s of the 100 MHz wall clock per wait
  a.stamps = p->fz_stamps;
  if ((rc = prof_mark(p, true))) return rc;
  const size_t lds = fos::fz_lds_bytes((int)p->n);
  switch ((int)(p->n / 2048)) {
    case 1: rc = launch_fused<1>(a, G, lds, p->stream); break;
    case 2: rc = launch_fused<2>(a, G, lds, p->stream); break;
    case 3: rc = launch_fused<3>(a, G, lds, p->stream); break;
    default: rc = launch_fused<4>(a, G, lds, p->stream); break;
  }
  if (rc) return rc;
  if ((rc = prof_mark(p, false))) return rc;
  const long long last = f->h_k - 1;
  const double* prev = iters >= 2 ? p->ws.fz_part + (size_t)((last - 1) & 1) * G * 4 : nullptr;
  if ((rc = finish_plain(f, p->ws.fz_part + (size_t)(last & 1) * G * 4, prev, G, p->pass.rr_part, G))) return rc;
  restart_plain(f, true);                          // the kernel leaves y_{k+iters} in ynext
  // a grid-wide wait that ran out leaves the state invalid: report it (synchronises)
  unsigned bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, p->ws.fz_bar + fos::FZ_LINE, sizeof(unsigned), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  if (bad) return fail(FOS_ERR_STATE, "fos_fista_run_fused: a grid-wide wait timed out (workgroups not co-resident?); state invalid");
  return FOS_OK;
}

// Tall-skinny plain runs with A resident in the LDS of up to all CUs, one grid barrier per iteration (chip_resident.hpp). Opt-in.
int fos_fista_run_chip(fos_fista* f, int iters) {
  if (!f || iters < 0) return fail(FOS_ERR_ARG, "fos_fista_run_chip: bad argument");
  if (int rc_ = need_squared(f->p, "fos_fista_run_chip")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_run_chip")) return rc_;
  fos_problem* p = f->p;
  const int nc = p->n <= 8 ? 8 : 16;
  const int64_t cap = fos::cr_rows_cap(nc);
  if (p->dtype != FOS_F32 || p->n > 16 || p->comm || p->m < 512 || p->m > cap * (int64_t)p->ncu)
    return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_chip: fp32 A, n <= 16, 512 <= m <= rows that fit the LDS of all CUs, unsharded");
  // plain runs take the momentum sequence from the host; adaptive restart and the step / ratio stops are decided on the device
  // by every workgroup alike (CTRL); the gradient-norm rule, the fp64 split gradient and a device-held step are not served
  if (f->precise || f->prm.tau_from_state || f->prm.tol_grad > 0.0)
    return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_chip: no gradient-norm rule, fp64 split gradient or device-held step (backtracking)");
  const bool ctrl = !plain_run(f);
  if (iters == 0) return FOS_OK;
  bool stopped = false;
  int rc = ctrl ? flush_pending(f) : begin_plain(f, &stopped);
  if (rc || stopped) return rc;
  // about 1024 rows (four per thread) per workgroup, at most what its LDS holds: the barrier, not the pass, is the cost, and it
  // grows with the number of workgroups (tools/bench_chip.py: 100000 x 5 took 11.9 us per iteration on 256 workgroups)
  int64_t G = std::max<int64_t>(1, std::min<int64_t>(p->ncu, (p->m + 1023) / 1024));
  G = std::max<int64_t>(G, std::min<int64_t>(p->ncu, (p->m + cap - 1) / cap));
  int64_t rpw = (p->m + G - 1) / G;
  if (rpw > cap) return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_chip: rows per workgroup exceed the LDS budget");
  G = (p->m + rpw - 1) / rpw;
  if (!p->ws.cr_part) {
    if ((rc = p->ws.cr_bar.reserve(fos::FZ_BAR_WORDS))) return rc;
    HIP_TRY(hipMemsetAsync(p->ws.cr_bar, 0, fos::FZ_BAR_WORDS * sizeof(unsigned), p->stream));
    if ((rc = p->ws.cr_part.reserve((size_t)2 * p->ncu * 17 + 16))) return rc;
  }
  Momentum before;
  if ((rc = momentum_sequence(f, iters, &before))) return rc;
  double* stats = p->ws.cr_part + (size_t)2 * p->ncu * 17;
  fos::ChipArgs a{};
  a.A = (const float*)p->A; a.lda = p->lda; a.b = p->b; a.m = p->m; a.n = (int)p->n; a.rows_per_wg = rpw;
  a.part = p->ws.cr_part; a.x_cur = f->x_cur; a.x_prev = f->x_prev; a.beta = p->ws.fz_beta; a.stats = stats; a.rr_out = stats + 8;
  a.bar = p->ws.cr_bar; a.iters = iters; a.prox_kind = f->prm.prox_kind;
  a.tau = f->prm.tau; a.alpha1 = f->prm.alpha1; a.alpha2 = f->prm.alpha2;
  a.timeout_ticks = 100000000ull * 2ull;
  if ((rc = prof_mark(p, true))) return rc;
  const size_t lds = fos::cr_lds_bytes(nc, rpw);
  a.scal = f->scal; a.prm = f->prm;
  if (ctrl) rc = nc == 8 ? launch_chip<8, true>(a, (int)G, lds, p->stream) : launch_chip<16, true>(a, (int)G, lds, p->stream);
  else rc = nc == 8 ? launch_chip<8, false>(a, (int)G, lds, p->stream) : launch_chip<16, false>(a, (int)G, lds, p->stream);
  if (rc) return rc;
  if ((rc = prof_mark(p, false))) return rc;
  // A grid-wide wait that ran out (workgroups not co-resident: another kernel held CUs for longer than the bound) ends the
  // launch BEFORE anything is written back: the iterate on the device is the one the call started from.  The handle's
  // momentum counters are put back, the barrier words cleared, and the caller is told - it can run the two-launch loop.
  unsigned bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, p->ws.cr_bar + fos::FZ_LINE, sizeof(unsigned), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  if (bad) {
    restore_momentum(f, before);
    HIP_TRY(hipMemsetAsync(p->ws.cr_bar, 0, fos::FZ_BAR_WORDS * sizeof(unsigned), p->stream));
    return fail(FOS_ERR_STATE, "fos_fista_run_chip: a grid-wide wait timed out (workgroups not co-resident); the state is "
                               "the one before the call");
  }
  if (ctrl) {                                      // the kernel advanced FistaScalars itself
    hand_to_device(f);
    return FOS_OK;
  }
  restart_plain(f);                                // ynext is not maintained here
  return finish_plain(f, stats, iters >= 2 ? stats + 4 : nullptr, 1, stats + 8, 1);
}

// The arguments of the lockstep update kernels: every state machine's buffers, weights, step and prox kind (bit v of
// prox_bits); plain runs also take its next momentum step (controlled runs take beta from the device scalars).
static fos::MultiUpdate multi_update(fos_fista* const* fs, int nv, bool controlled) {
  fos::MultiUpdate mu{};
  for (int v = 0; v < nv; ++v) {
    fos_fista* f = fs[v];
    mu.x_cur[v] = f->x_cur; mu.x_prev[v] = f->x_prev; mu.scal[v] = f->scal; mu.part[v] = f->part2;
    mu.alpha1[v] = f->prm.alpha1; mu.alpha2[v] = f->prm.alpha2; mu.tau[v] = f->prm.tau;
    mu.prox_bits |= (f->prm.prox_kind == fos::PROX_ENET ? 1 : 0) << v;
    if (!controlled) {
      const PlainStep s = advance_plain(f, false);
      mu.part[v] = s.part; mu.beta[v] = s.beta; mu.beta_next[v] = s.beta_next;
    }
  }
  return mu;
}

// Up to 16 state machines in lockstep on the matrix cores (gram_batch.hpp): per iteration and per row panel, product 1
// (R = A_panel Y - b, from HBM) and product 2 (G += R^T A_panel, the panel again from the Infinity Cache), then the updates,
// which leave every y_{k+1} in the candidate block of the next product 1.  The layout: plan_multi_mfma (fos_plan.hip).
// The separable update is one launch for all state machines (launch_separable_update), whatever their families.
// b16 (several right-hand sides, unsharded): product 1 subtracts column j of this m x 16 block from candidate column j
// instead of the problem's b; always the two-product form (the planner's cluster layout, if any, is left as it is).
// fold_of_row / held (K-fold cross-validation, unsharded, the problem's own b): product 1 zeroes column j's residual on the
// rows of the fold it holds out (batch_trial.hpp FOLD_TRAIN), so state machine j fits the other rows; the two-product form
// likewise.  Product 2 and the updates see a masked R and are the same launches.
// A logistic problem (fos_problem_set_loss): product 1 is the logistic form, R = sigma(A_panel Y) - b with or without the fold
// mask; the two-product form as well, and everything after product 1 is the same.
// A problem with row weights (fos_row_weights_bind): product 1 is the weighted form of its loss, R = w (A_panel Y - b) or
// w (sigma(A_panel Y) - b); the two-product form, and everything after product 1 is the same.
// A problem with coordinate data (fos_coord_bind: penalty factors and box bounds): the two-product form as well; both products
// are the launches they were and the separable update launch takes the coordinate form (reduce_update.hpp, COORD), which
// scales the penalties per coordinate and clamps to the box.  Composes with the fold mask, the logistic loss and row weights.
// A multinomial problem (fos_problem_set_multinomial): the 16 columns are the class vectors of floor(16 / C) joint fits.
// Product 1 is the plain storing form, R = A_panel Y (the logits; neither b nor a mask nor the weights enter it), the link
// kernel (softmax_link.hpp) turns the panel into softmax(A_panel Y) - onehot(b) in place with the weights and the fold mask
// applied, and everything after it is the same.  Plain runs only (lockstep_route).
// A Huber or squared-hinge problem (fos_problem_set_link_loss): the same sequence with the pointwise link kernel
// (pointwise_link.hpp), R = clip(A_panel Y - b, -c, c) or -b max(0, 1 - b A_panel Y).  The columns are independent fits: any nv,
// plain or controlled.
// A resample of the rows per column (fos_fista_run_multi_resampled: counts, a nibble per row and column): the same sequence on
// any of the four losses above with the resample link kernel (resample_link.hpp), which forms the loss's residual itself and
// multiplies it by the bound weight and the column's multiplicity; any nv, plain or controlled.

// Handles under the group penalty (fos_fista_params.group = G >= 2; checked by group_refusal before they get here): always the
// two-product form, plain; the G columns of a fit are updated together by the one launch of launch_group_update, in place of
// the separable update.  Penalty factors compose (the factor of a coordinate scales its row's threshold); box bounds do not
// and are refused.

// Row splits of product 2 in the two-product form: the planned ones, or - on a problem planned for the cluster form, whose slab
// count is the number of clusters - the two-product splits, which must fit the slabs the cluster form allocated.
static int two_product_splits(const fos_problem* p, int* g_splits) {
  *g_splits = p->multi.gram_splits;
  if (p->multi.cp_cs) {
    *g_splits = (int)((p->multi.panel_rows + p->multi.gram_rows_per_split - 1) / p->multi.gram_rows_per_split);
    if (*g_splits > p->multi.gram_splits)
      return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_multi_rhs / _folds / logistic loss / row weights: the cluster layout of this "
                                       "problem has too few slabs for the two-product form");
  }
  return FOS_OK;
}

// Product 2 on one row panel (run_multi_mfma, fos_gram_apply): slabs16[split][16][n] (+)= R_panel^T A_panel, the panel again
// from the Infinity Cache.
static int launch_gram_panel(fos_problem* p, const char* Ap, int64_t rows, int g_splits, bool accumulate) {
  const bool is_bf16 = p->dtype == FOS_BF16;
  const int64_t strips = (p->n + (is_bf16 ? fos::GQ_COLS : fos::GB_COLS) - 1) / (is_bf16 ? fos::GQ_COLS : fos::GB_COLS);
  const dim3 grid((unsigned)strips, (unsigned)g_splits);
#define FOS_GRAM(T, ACC)                                                                                                  \
  hipLaunchKernelGGL((fos::gram_batch_mfma_kernel<T, ACC>), grid, dim3(fos::GB_THREADS), 0, p->stream, (const T*)Ap, p->lda, \
                     rows, (int)p->n, p->multi.rbuf16, p->multi.gram_rows_per_split, p->multi.slabs16, p->n)
  if (is_bf16) {
    if (accumulate)
      hipLaunchKernelGGL(fos::gram_batch_mfma_bf16_kernel<true>, grid, dim3(fos::GB_THREADS), 0, p->stream,
                         (const fos::bf16_t*)Ap, p->lda, rows, (int)p->n, p->multi.rbuf16, p->multi.gram_rows_per_split, p->multi.slabs16, p->n);
    else
      hipLaunchKernelGGL(fos::gram_batch_mfma_bf16_kernel<false>, grid, dim3(fos::GB_THREADS), 0, p->stream,
                         (const fos::bf16_t*)Ap, p->lda, rows, (int)p->n, p->multi.rbuf16, p->multi.gram_rows_per_split, p->multi.slabs16, p->n);
  } else { if (accumulate) FOS_GRAM(float, true); else FOS_GRAM(float, false); }
#undef FOS_GRAM
  LAUNCH_CHECK();
  return FOS_OK;
}

// The update of nv / G joint fits under the group penalty in one launch (fista_update_group_kernel): grid (nupd, nv / G).
static int launch_group_update(fos_fista* const* fs, int nv, int g_splits, int y_mode) {
  fos_problem* p = fs[0]->p;
  const int G = fs[0]->prm.group;
  const fos::MultiUpdate mu = multi_update(fs, nv, false);
  hipLaunchKernelGGL(fos::fista_update_group_kernel, dim3(fs[0]->nupd, nv / G), dim3(256), 0, p->stream, p->multi.slabs16, g_splits,
                     (int)p->n, mu, G, p->cand.xp, y_mode, p->coord_factor);
  LAUNCH_CHECK();
  return FOS_OK;
}

// The update on a problem with feature groups (fos_feature_groups_bind) in three launches (reduce_update.hpp): u and the
// gradient partial over (nupd, nv), the group norms with one wave per (group, column), the scaling over (nupd, nv) again.  One
// MultiUpdate serves all three: a plain run's momentum step is advanced once.
static int launch_fgroup_update(fos_fista* const* fs, int nv, int g_splits, int y_mode, bool controlled) {
  fos_problem* p = fs[0]->p;
  const fos::MultiUpdate mu = multi_update(fs, nv, controlled);
  const fos::FeatureGroupData fg{p->fg.start, p->fg.weight, p->fg.of_coord, p->fg.u, p->fg.nrm2, p->fg.ngroups, (p->n + 3) / 4 * 4,
                                 p->fg.l1_mix};
  const int host_beta = controlled ? 0 : 1;
  hipLaunchKernelGGL(fos::fgroup_form_u_kernel, dim3(fs[0]->nupd, nv), dim3(256), 0, p->stream, p->multi.slabs16, g_splits, (int)p->n,
                     mu, host_beta, fg);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(fos::fgroup_norm_kernel, dim3((fg.ngroups + fos::FG_WAVES - 1) / fos::FG_WAVES, nv), dim3(64 * fos::FG_WAVES), 0,
                     p->stream, mu, fg);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(fos::fgroup_scale_kernel, dim3(fs[0]->nupd, nv), dim3(256), 0, p->stream, (int)p->n, mu, p->cand.xp, y_mode,
                     host_beta, fg);
  LAUNCH_CHECK();
  return FOS_OK;
}

// The separable update of all nv state machines in ONE launch (fista_update_multi_kernel), grid (nupd, nv): one family or
// mixed families (the prox kind travels per column), plain or controlled, with or without coordinate data.
static int launch_separable_update(fos_fista* const* fs, int nv, int g_splits, int y_mode, bool controlled) {
  fos_problem* p = fs[0]->p;
  const fos::MultiUpdate mu = multi_update(fs, nv, controlled);
  const fos::CoordData cd{p->coord_factor, p->coord_lo, p->coord_hi};
  auto kern = has_coord(p) ? fos::fista_update_multi_kernel<true> : fos::fista_update_multi_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(fs[0]->nupd, nv), dim3(256), 0, p->stream, p->multi.slabs16, g_splits, (int)p->n, mu, p->cand.xp,
                     y_mode, controlled ? 0 : 1, cd);
  LAUNCH_CHECK();
  return FOS_OK;
}

// The resample link kernel (resample_link.hpp) behind product 1 on one row panel: the `rows` rows of p->multi.rbuf16 that product
// 1 in its plain storing form has just filled with Z of the panel starting at row0.  counts: the words of ALL rows (offset by
// row0 here, as b and the weights are).  gram: the loss-free form R = (w c) z; else the problem's loss.  oob: only the
// out-of-bag sums, R is left as it is.  One lane per 16-byte quad of a row, grid-stride: at most 2 * ncu workgroups, within the
// 3 * ncu + 8 rows of cand.q_part; *nwg_out = the rows of q_part written (0 in the Gram form, which has no sums).
static int launch_resample_link(fos_problem* p, bool gram, int64_t row0, int64_t rows, int nv, const uint64_t* counts, int oob,
                                double* q_part, int* nwg_out) {
  if (!counts || rows < 1 || rows > p->multi.panel_rows || row0 < 0 || row0 + rows > p->m || nv < 1 || nv > fos::BT_NV ||
      (gram ? oob != 0 : (!p->b || !q_part)))
    return fail(FOS_ERR_STATE, "launch_resample_link: not a panel of a resampled pass");
  const int nwg = (int)std::min<int64_t>((4 * rows + fos::RL_THREADS - 1) / fos::RL_THREADS, 2 * (int64_t)p->ncu);
  const float* w = p->row_weight ? p->row_weight + row0 : nullptr;
  const float* b = gram ? nullptr : p->b + row0;
  const uint16_t* c16 = reinterpret_cast<const uint16_t*>(counts + row0);
  const float c = (float)p->link_param;
#define FOS_RESAMPLE(K, M, W)                                                                                                  \
  hipLaunchKernelGGL((fos::resample_link_kernel<fos::K, fos::M, W>), dim3(nwg), dim3(fos::RL_THREADS), 0, p->stream,           \
                     p->multi.rbuf16.get(), rows, b, c, nv, w, c16, q_part, (const int*)nullptr)
#define FOS_RESAMPLE_FORM(K)                                                                                      \
  {                                                                                                               \
    if (oob) { if (w) FOS_RESAMPLE(K, RESAMPLE_OOB, true); else FOS_RESAMPLE(K, RESAMPLE_OOB, false); }           \
    else { if (w) FOS_RESAMPLE(K, RESAMPLE_INBAG, true); else FOS_RESAMPLE(K, RESAMPLE_INBAG, false); }           \
  }
  if (gram) { if (w) FOS_RESAMPLE(RESAMPLE_GRAM, RESAMPLE_INBAG, true); else FOS_RESAMPLE(RESAMPLE_GRAM, RESAMPLE_INBAG, false); }
  else switch (p->loss) {
    case FOS_LOSS_SQUARED: FOS_RESAMPLE_FORM(RESAMPLE_SQUARED) break;
    case FOS_LOSS_LOGISTIC: FOS_RESAMPLE_FORM(RESAMPLE_LOGISTIC) break;
    case FOS_LOSS_HUBER: FOS_RESAMPLE_FORM(RESAMPLE_HUBER) break;
    case FOS_LOSS_SQUARED_HINGE: FOS_RESAMPLE_FORM(RESAMPLE_SQUARED_HINGE) break;
    default: return fail(FOS_ERR_STATE, "launch_resample_link: the loss has no resampled form");
  }
#undef FOS_RESAMPLE_FORM
#undef FOS_RESAMPLE
  LAUNCH_CHECK();
  *nwg_out = gram ? 0 : nwg;
  return FOS_OK;
}

// One call of a lockstep entry point, as its arguments came in (checked), and what lockstep_route decides for it.
struct LockstepCall {
  fos_fista* const* fs;
  int nv, iters;
  const float* B;                    // fos_fista_run_multi_rhs: column v of this m x nv block for state machine v (null: the problem's b)
  int64_t ldb;
  const uint8_t* fold_of_row;        // fos_fista_run_multi_folds: the fold of every row, the HOST held ids and their block (null: no mask)
  const int32_t* held_ids;
  const fos::FoldHeld* held;
  const char* fn;                    // the entry point, for messages
  const uint64_t* counts = nullptr;  // fos_fista_run_multi_resampled: the multiplicity words of all rows (null: every row once)
};
enum LockstepEngine { ENGINE_SINGLE, ENGINE_VALU, ENGINE_MFMA };
struct LockstepRoute {
  LockstepEngine engine;             // fos_fista_run on the one handle, the VALU multi-vector pass, the matrix-core pair
  MultiLaunch valu;                  // ENGINE_VALU: its kernel
  bool controlled;                   // momentum and stops decided on the device, per state machine
  bool same_family;                  // the state machines share mode / prox kind / delta (what the lockstep bookkeeping takes from fs[0])
  bool stage_b;                      // B is staged into p->ws.b16 before the engine runs
};

static int run_multi_mfma(const LockstepCall& c, const LockstepRoute& r) {
  fos_fista* const* fs = c.fs;
  const int nv = c.nv, iters = c.iters;
  const bool controlled = r.controlled;
  const uint8_t* fold_of_row = c.fold_of_row;
  const fos::FoldHeld* held = c.held;
  fos_problem* p = fs[0]->p;
  const float* b16 = r.stage_b ? p->ws.b16.get() : nullptr;
  const bool cols = p->col_sharded;
  if (cols && !controlled) return fail(FOS_ERR_STATE, "run_multi_mfma: a column-sharded lockstep is device-controlled");
  assert(!controlled || r.same_family);       // the bookkeeping kernels take mode / delta from fs[0] (lockstep_route refuses the rest)
  int rc = ensure_batch_workspace(p);
  if (rc) return rc;
  if (cols && (rc = p->ws.mfold.reserve((size_t)fos::BT_NV * 4))) return rc;
  if ((rc = plan_multi_mfma(p))) return rc;
  const bool is_bf16 = p->dtype == FOS_BF16;
  const int64_t esz = is_bf16 ? 2 : 4;
  const int y_mode = is_bf16 ? fos::YOUT_XQ : fos::YOUT_XP;
  const bool logit = p->loss == FOS_LOSS_LOGISTIC;
  const bool weighted = p->row_weight != nullptr;
  const bool softmax = p->loss == FOS_LOSS_MULTINOMIAL;      // the link kernel sits between the two products of every panel
  const bool link = link_loss(p);                            // the pointwise link kernel, in the same place
  const bool group_penalty = grouped(fs[0]->prm);            // the fits' columns are updated together (launch_group_update)
  const bool fgroup = has_fgroups(p);                        // fos_feature_groups_bind: the update is launch_fgroup_update
  const bool two_products = b16 || fold_of_row || logit || weighted || has_coord(p) || group_penalty || fgroup;
  const uint64_t* counts = c.counts;                         // a resample per column: the resample link kernel, in the same place
  bool use_cluster = p->multi.cp_cs && !two_products && !softmax && !link && !counts;
  int g_splits = p->multi.gram_splits;
  if ((two_products || softmax || link) && (rc = two_product_splits(p, &g_splits))) return rc;
  if (counts && (rc = two_product_splits(p, &g_splits))) return rc;
  // candidate block: zero everywhere (padding columns, unused slots), then y_k of every state machine
  const size_t per_entry = is_bf16 ? 3 * sizeof(unsigned short) : sizeof(float);
  HIP_TRY(hipMemsetAsync(p->cand.xp, 0, (size_t)p->cand.n_pad * fos::BT_NV * per_entry, p->stream));
  // Controlled run (adaptive restart / step or ratio tolerance on any weight): momentum and stops are decided on the
  // device per state machine, every iteration; a stopped weight is a masked column of the block.
  fos::MultiControl mc{};
  if (controlled) {
    for (int v = 0; v < nv; ++v) {
      fos_fista* f = fs[v];
      if ((rc = flush_pending(f))) return rc;
      hand_to_device(f);
      mc.scal[v] = f->scal; mc.part[v] = f->part2; mc.x_cur[v] = f->x_cur; mc.x_prev[v] = f->x_prev;
      mc.adaptive_restart[v] = f->prm.adaptive_restart; mc.restart_threshold[v] = f->prm.restart_threshold;
      mc.tol_step[v] = f->prm.tol_step; mc.tol_ratio[v] = f->prm.tol_ratio;
    }
    hipLaunchKernelGGL(fos::form_y_multi_kernel, dim3(grid_1d(p->n, 256, 64), nv), dim3(256), 0, p->stream, mc, (int)p->n, p->cand.xp,
                       y_mode, 1);
    LAUNCH_CHECK();
  }
  for (int v = 0; v < nv && !controlled; ++v) {
    fos_fista* f = fs[v];
    bool stopped = false;
    if ((rc = begin_plain(f, &stopped))) return rc;
    if (stopped) return fail(FOS_ERR_STATE, "fos_fista_run_multi: a handle has already stopped");
    hipLaunchKernelGGL(fos::form_y_block_kernel, dim3(grid_1d(p->n, 256, 256)), dim3(256), 0, p->stream, f->x_cur, f->x_prev,
                       f->h_beta, (int)p->n, v, p->cand.xp, y_mode);
    LAUNCH_CHECK();
    restart_plain(f);                // y lives in the candidate block; part2 partials are counted from this run on
  }
  for (int it = 0; it < iters; ++it) {
    if ((rc = prof_mark(p, true))) return rc;
    if (use_cluster && (rc = launch_cluster_pass(p))) {
      if (p->cp_mode == 1 || it > 0) return rc;
      (void)hipGetLastError();                   // planner's own choice refused (cooperative launch): two products instead
      p->cp_mode = 2;
      if ((rc = invalidate(p, IN_CLUSTER)) || (rc = plan_multi_mfma(p))) return rc;
      use_cluster = false;
      g_splits = p->multi.gram_splits;
    }
    for (int64_t row0 = 0, panel = 0; !use_cluster && row0 < p->m; row0 += p->multi.panel_rows, ++panel) {
      const int64_t rows = std::min<int64_t>(p->multi.panel_rows, p->m - row0);
      const char* Ap = reinterpret_cast<const char*>(p->A) + (size_t)row0 * p->lda * esz;
      int nwg1 = 0;
      // column-sharded: b enters the sum over the ranks once (rank 0); R = sum_p A_p Y_p - b is the ONE exchange per panel
      const float* bp = b16 ? b16 + row0 * fos::BT_NV : (p->b && !(cols && p->comm->rank != 0)) ? p->b + row0 : nullptr;
      // a fold mask, the logistic loss and row weights read the problem's own b (the labels); fold ids and weights are offset
      // with the panel as b is (panel rows are a multiple of 256)
      BatchLaunch L{};
      L.A = Ap; L.b = (fold_of_row || logit || weighted) ? p->b + row0 : bp; L.use_b = 1; L.rows = rows; L.rout = p->multi.rbuf16;
      L.bblock = b16 != nullptr; L.fold_of_row = fold_of_row ? fold_of_row + row0 : nullptr; L.held = held;
      L.row_weight = weighted ? p->row_weight + row0 : nullptr;
      if (softmax) { L.b = nullptr; L.use_b = 0; L.fold_of_row = nullptr; L.held = nullptr; L.row_weight = nullptr; }     // the logits alone
      if (link) { L.b = nullptr; L.use_b = 0; L.fold_of_row = nullptr; L.held = nullptr; L.row_weight = nullptr; }        // A_panel Y alone
      if (counts) { L.b = nullptr; L.use_b = 0; L.bblock = false; L.row_weight = nullptr; }       // likewise, whatever the loss
      if ((rc = launch_batch_product(p, L, &nwg1))) return rc;
      if (counts && (rc = launch_resample_link(p, false, row0, rows, nv, counts, 0, p->cand.q_part, &nwg1))) return rc;
      if (softmax && (rc = launch_softmax_link(p, row0, rows, nv, fold_of_row ? fos::FOLD_TRAIN : fos::FOLD_OFF, fold_of_row, held,
                                               p->cand.q_part, &nwg1)))
        return rc;
      if (link && !counts && (rc = launch_pointwise_link(p, row0, rows, nv, fold_of_row ? fos::FOLD_TRAIN : fos::FOLD_OFF, fold_of_row, held,
                                                         p->cand.q_part, &nwg1)))
        return rc;
      if (cols && (rc = reduce_across(p, p->multi.rbuf16, (size_t)rows * fos::BT_NV, false))) return rc;
      if ((rc = launch_gram_panel(p, Ap, rows, g_splits, panel != 0))) return rc;
    }
    if ((rc = prof_mark(p, false))) return rc;
    // row-sharded problem: the 16 partial gradients (all row splits) are summed over the ranks before the updates
    // (column-sharded: the gradient block is local)
    if (!cols && (rc = reduce_across(p, p->multi.slabs16, (size_t)g_splits * fos::BT_NV * p->n, false))) return rc;
    // the update stage: feature groups - three launches; the group penalty - one; everything else - the one separable launch
    if (fgroup) rc = launch_fgroup_update(fs, nv, g_splits, y_mode, controlled);      // (never with group_penalty)
    else if (group_penalty) rc = launch_group_update(fs, nv, g_splits, y_mode);
    else rc = launch_separable_update(fs, nv, g_splits, y_mode, controlled);
    if (rc) return rc;
    if (controlled) {                            // bookkeeping of all weights (device beta) -> their y_{k+1}
      if (cols) {                                // step norms, ||x||^2, ||x||_1 are sums over the column blocks of all ranks
        hipLaunchKernelGGL(fold4_multi_kernel, dim3(nv), dim3(64), 0, p->stream, mc, fs[0]->nupd, p->ws.mfold);
        LAUNCH_CHECK();
        if ((rc = reduce_across(p, p->ws.mfold, (size_t)nv * 4, true))) return rc;
        fos::MultiControl mf = mc;
        for (int v = 0; v < nv; ++v) mf.part[v] = p->ws.mfold + (size_t)v * 4;
        hipLaunchKernelGGL(fos::fista_finalize_multi_kernel, dim3(nv), dim3(64), 0, p->stream, mf, 1, fs[0]->prm);
      } else
        hipLaunchKernelGGL(fos::fista_finalize_multi_kernel, dim3(nv), dim3(64), 0, p->stream, mc, fs[0]->nupd, fs[0]->prm);
      LAUNCH_CHECK();
      hipLaunchKernelGGL(fos::form_y_multi_kernel, dim3(grid_1d(p->n, 256, 64), nv), dim3(256), 0, p->stream, mc, (int)p->n, p->cand.xp,
                         y_mode, 0);
      LAUNCH_CHECK();
    }
  }
  if (use_cluster) {     // a cluster member that waited out its bound parked itself and raised the flag: the sums are invalid
    int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, p->multi.cp_error, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (bad) return fail(FOS_ERR_STATE, "fos_fista_run_multi: the one-read cluster pass timed out waiting for a member "
                                        "(results invalid); rerun with FOS_PLAN_NO_CLUSTER");
  }
  for (int v = 0; v < nv && !controlled; ++v) {
    if ((rc = finish_part2(fs[v], 0))) return rc;
    restart_plain(fs[v]);            // the next single-vector run counts its part2 partials afresh
  }
  return FOS_OK;
}

// ---- The route decision of the lockstep: which engine serves a call of fos_fista_run_multi / _rhs / _folds, or why none does ----
static bool any_grouped(fos_fista* const* fs, int nv) {
  for (int v = 0; v < nv; ++v)
    if (grouped(fs[v]->prm)) return true;
  return false;
}

// Handle v carries the parameters of the first handle of its fit (`width` consecutive columns: G, or the class count) and,
// with held ids, holds out the same fold.  The caller words the refusal.
static bool fit_column_agrees(fos_fista* const* fs, int v, int width, const int32_t* held) {
  const int v0 = v / width * width;
  const fos::FistaParams &a = fs[v0]->prm, &c = fs[v]->prm;
  return a.group == c.group && a.tau == c.tau && a.alpha1 == c.alpha1 && a.alpha2 == c.alpha2 && a.delta == c.delta &&
         a.mode == c.mode && a.prox_kind == c.prox_kind && !(held && held[v] != held[v0]);
}

// What everything but the plain squared loss needs: the problem's own b, no sharding, the matrix-core pair.
static bool unsharded_pair(const fos_problem* p) { return !p->comm && !p->col_sharded && pair_dd_multi_supported(p); }

// What the lockstep serves under the group penalty (fos_fista_params.group = G >= 2), checked before any launch or change of
// handle state; FOS_OK without a grouped handle.  All handles are grouped with one G, nv is a multiple of G, the G handles of a
// fit carry identical parameters and hold out one fold (held: HOST ids or null), every handle is a plain run without the fp64
// split gradient or a device-held step, G is the class count of a multinomial problem, no box bound is bound (group norm plus
// box has no composed closed-form prox; penalty factors alone compose) and the problem is unsharded with the matrix-core pair.
static int group_refusal(fos_fista* const* fs, int nv, const int32_t* held, const char* fn) {
  bool any = false, all = true;
  for (int v = 0; v < nv; ++v) { any = any || grouped(fs[v]->prm); all = all && grouped(fs[v]->prm); }
  if (!any) return FOS_OK;
  const fos_problem* p = fs[0]->p;
  const int G = fs[0]->prm.group;
  const char* why = nullptr;
  if (!all) why = "grouped and ungrouped handles do not mix in one call";
  else if (nv % G != 0) why = "nv is a multiple of the group size";
  for (int v = 0; v < nv && !why; ++v) {
    const fos_fista* f = fs[v];
    if (!fit_column_agrees(fs, v, G, held))
      why = "the handles of a group carry identical parameters and hold out one fold";
    else if (!plain_run(f) || f->precise || f->prm.tau_from_state)
      why = "plain runs only (no adaptive restart, no step / ratio / gradient tolerance, no fp64 split gradient, no device-held "
            "step: a rule decided per column would break the joint fit)";
  }
  if (!why && p->loss == FOS_LOSS_MULTINOMIAL && G != p->classes) why = "on a multinomial problem the group size is the class count";
  if (!why && (p->coord_lo || p->coord_hi))
    why = "box bounds (fos_coord_bind) do not compose with the group norm; penalty factors alone do";
  if (!why && !unsharded_pair(p)) why = "an unsharded problem with the matrix-core pair is needed";
  if (!why && has_fgroups(p)) why = "feature groups (fos_feature_groups_bind) are bound; the two group norms do not compose";
  if (!why && link_loss(p)) why = "not served with the Huber or the squared-hinge loss (fos_problem_set_link_loss)";
  if (why) return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": the group penalty (fos_fista_params.group >= 2): " + why);
  return FOS_OK;
}

// fos_fista_run_multi_rhs: grouped handles on an unweighted squared-loss problem (with or without coordinate data) pass its
// need_squared - penalty factors compose with the group penalty, and group_refusal refuses bounds itself
static bool group_takes_block(fos_fista* const* fs, int nv) {
  return any_grouped(fs, nv) && fs[0]->p->loss == FOS_LOSS_SQUARED && fs[0]->p->row_weight == nullptr;
}

// Fills *r from the call, or refuses it; launches nothing and touches neither a handle nor device state.  In order: the
// multinomial loss, the group penalty, the logistic loss / row weights / coordinate data / feature groups (all on the
// matrix-core pair, for any number of state machines - there is no single-vector or VALU pass for them; a block B met
// need_squared), the Huber / squared-hinge loss (the pair likewise), the fold masks on the squared loss, and the squared loss on its own b or on B.
static int lockstep_route(const LockstepCall& c, LockstepRoute* r) {
  fos_fista* const* fs = c.fs;
  const int nv = c.nv;
  fos_problem* p = fs[0]->p;
  const std::string fn = c.fn;
  const bool rhs = c.B != nullptr;
  bool all_plain = true, controllable = true, same_family = true;
  for (int v = 0; v < nv; ++v) {
    all_plain = all_plain && plain_run(fs[v]);
    // what the lockstep bookkeeping decides on the device: adaptive restart, step and ratio tolerances (the gradient-norm
    // rule sits BEFORE the update and backtracking needs its own candidates per weight: those run one by one)
    controllable = controllable && fs[v]->prm.tol_grad == 0.0 && !fs[v]->precise && !fs[v]->prm.tau_from_state;
    const fos::FistaParams &a = fs[0]->prm, &q = fs[v]->prm;
    same_family = same_family && a.mode == q.mode && a.prox_kind == q.prox_kind && a.delta == q.delta;
  }
  // the matrix-core pair for whatever follows, unless a squared-loss decision below says otherwise
  *r = LockstepRoute{ENGINE_MFMA, nullptr, !all_plain, same_family, rhs};
  // device control (adaptive restart, step / ratio stops) is the bookkeeping of ONE family, and nothing else is decided there
  auto control_refusal = [&]() {
    if (!controllable) return fail(FOS_ERR_UNSUPPORTED, fn + ": no gradient-norm rule, fp64 split gradient or device-held step");
    if (!all_plain && !same_family) return fail(FOS_ERR_UNSUPPORTED, fn + ": a device-controlled lockstep serves one family");
    return (int)FOS_OK;
  };
  if (p->loss == FOS_LOSS_MULTINOMIAL) {
    // nv / C joint fits of C columns each.  A stop or restart decided per column would break a joint fit, so only plain runs
    // are served, and the columns of a fit share their parameters (and the fold they hold out).
    if (int rc = group_refusal(fs, nv, c.held_ids, c.fn)) return rc;     // the grouped form: G = C, no bounds, one G for all
    if (!p->b || !unsharded_pair(p))
      return fail(FOS_ERR_UNSUPPORTED, fn + ": the multinomial loss needs b, an unsharded problem and the matrix-core pair");
    if (!softmax_groups_ok(p, nv, c.held_ids))
      return fail(FOS_ERR_UNSUPPORTED, fn + ": on a multinomial problem nv is a multiple of the classes and the handles of "
                                            "a class group hold out one fold");
    if (int rc = control_refusal()) return rc;
    if (!all_plain)
      return fail(FOS_ERR_UNSUPPORTED, fn + ": a multinomial problem is served plain runs only (no adaptive restart, no "
                                            "step or ratio tolerance: a rule decided per column would break the joint fit)");
    for (int v = 0; v < nv; ++v)
      if (!fit_column_agrees(fs, v, p->classes, nullptr))
        return fail(FOS_ERR_UNSUPPORTED, fn + ": the handles of a class group of a multinomial problem carry identical "
                                              "parameters");
    return FOS_OK;
  }
  if (any_grouped(fs, nv)) {
    // nv / G fits of G columns each, for any nv (nv == G == 2 included).  B (the targets of a multi-task fit) is taken by
    // product 1 for the unweighted squared loss alone.
    if (int rc = group_refusal(fs, nv, c.held_ids, c.fn)) return rc;
    if (rhs ? (p->loss != FOS_LOSS_SQUARED || p->row_weight != nullptr)
            : (!p->b && (c.fold_of_row || p->loss != FOS_LOSS_SQUARED || p->row_weight)))
      return fail(FOS_ERR_UNSUPPORTED, fn + ": the group penalty (fos_fista_params.group >= 2): a right-hand-side block "
                                            "needs the unweighted squared loss, everything else the problem's own b");
    return FOS_OK;
  }
  if (link_loss(p)) {
    // independent columns behind a pointwise link (group_refusal has refused the group penalty): any nv, plain or controlled,
    // refused as on a logistic problem otherwise
    if (!p->b || !unsharded_pair(p))
      return fail(FOS_ERR_UNSUPPORTED, fn + ": the Huber and squared-hinge losses need b, an unsharded problem and the "
                                            "matrix-core pair");
    return control_refusal();
  }
  if (p->loss == FOS_LOSS_LOGISTIC || p->row_weight || has_coord(p) || has_fgroups(p)) {
    if (!p->b || !unsharded_pair(p))
      return fail(FOS_ERR_UNSUPPORTED, fn + ": the logistic loss, row weights and penalty factors / bounds need b, an unsharded problem and the "
                                            "matrix-core pair");
    return control_refusal();
  }
  // a resample per column (fos_fista_run_multi_resampled, which has refused what the pair does not serve: resample_refusal) on
  // the plain squared loss: the pair for any nv, as the link kernel sits between its products
  if (c.counts) return control_refusal();
  if (c.fold_of_row) {
    // always the two matrix-core products, for any number of state machines: the alternative is a copy of A per fold
    if (!p->b) return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_multi_folds: the problem has no b of its own");
    if (p->comm || p->col_sharded)
      return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_multi_folds: row- or column-sharded problems are not served");
    if (!pair_dd_multi_supported(p))
      return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_multi_folds: the shape has no matrix-core pair");
    return control_refusal();
  }
  // the squared loss on the problem's b, or on the columns of B
  if (rhs && (p->comm || p->col_sharded))
    return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_multi_rhs: row- or column-sharded problems are not served");
  if (nv == 1) {
    if (rhs) return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_multi_rhs: one column runs as a problem of its own");
    r->engine = ENGINE_SINGLE;
    return FOS_OK;
  }
  const bool shape_ok = batch_supported(p) && !p->pass.colblock && !p->pass.resident && !p->col_sharded;
  // Column-sharded (very wide A): the two products per panel with ONE exchange of the panel's 16 residual columns between
  // them; always device-controlled (step norms are sums over the ranks).  The matrix-core kernels tile any width.
  if (p->col_sharded) {
    if (!(controllable && same_family))
      return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_multi: a column-sharded lockstep serves one family without the "
                                       "gradient-norm rule / fp64 gradient / persisted step");
    r->controlled = true;
    return FOS_OK;
  }
  // the two-product pass costs about two single-vector passes per iteration whatever the number of weights: it pays
  // from three weights on (profiles/r02_multilambda.md); two weights without a VALU multi-vector kernel run one by one
  // (a sharded problem takes the matrix-core pass for any number of weights: its 16 gradients are one 16 x n all-reduce)
  const bool pair_pays = shape_ok && p->pass.entry != wide_entry(p->dtype) && (nv >= 3 || p->comm);
  if (!all_plain && controllable && same_family && pair_pays) return FOS_OK;
  const bool streaming = shape_ok && all_plain;
  r->valu = (streaming && !p->pass.tall && !p->comm && p->dtype == FOS_F32 && p->pass.entry != wide_entry(p->dtype)) ? find_multi(p->n, nv, rhs) : nullptr;
  if (!r->valu && streaming && pair_pays) return FOS_OK;          // 5..16 weights, n up to 16384, fp32 and bf16
  if (!r->valu) return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_multi: no multi-vector kernel for this shape / configuration");
  r->engine = ENGINE_VALU;
  return FOS_OK;
}

// The VALU multi-vector pass (gemv_multi.hpp): 2..4 plain fp32 state machines, one pass over A for all, an update per handle
// (their y are vectors of their own).
static int run_multi_valu(const LockstepCall& c, const LockstepRoute& r) {
  fos_fista* const* fs = c.fs;
  const int nv = c.nv;
  fos_problem* p = fs[0]->p;
  int rc;
  // workspace: nv interleaved slab sets and rr partials per workgroup
  const int nwg = p->pass.nwg;
  if ((rc = p->pass.slabs.reserve((size_t)nwg * nv * p->n)) || (rc = p->pass.rr_part.reserve((size_t)nwg * nv)) ||
      (rc = p->pass.rr2_part.reserve((size_t)nwg * nv)))
    return rc;
  fos::MultiY ys{};
  ys.stopped = nullptr;
  for (int v = 0; v < nv; ++v) {
    fos_fista* f = fs[v];
    bool stopped = false;
    if ((rc = begin_plain(f, &stopped))) return rc;
    if (stopped) return fail(FOS_ERR_STATE, "fos_fista_run_multi: a handle has already stopped");
    if ((rc = ensure_y(f))) return rc;
    ys.y[v] = f->ynext;
  }
  for (int v = nv; v < 4; ++v) ys.y[v] = ys.y[0];
  for (int it = 0; it < c.iters; ++it) {
    if ((rc = prof_mark(p, true))) return rc;
    r.valu((const float*)p->A, p->lda, r.stage_b ? p->ws.b16 : p->b, p->m, (int)p->n, ys, p->pass.rows_per_wg, p->pass.slabs, p->pass.rr_part, nwg, p->stream);
    LAUNCH_CHECK();
    if ((rc = prof_mark(p, false))) return rc;
    for (int v = 0; v < nv; ++v) {
      const PlainStep s = advance_plain(fs[v], true);
      if ((rc = launch_update_from_slabs(fs[v], s.part, 1, s.beta, nullptr, fs[v]->ynext, s.beta_next, p->pass.slabs + (size_t)v * p->n,
                                         (int64_t)nv * p->n)))
        return rc;
    }
  }
  for (int v = 0; v < nv; ++v)
    if ((rc = finish_part2(fs[v], 0))) return rc;
  return FOS_OK;
}

// A lockstep call behind its argument checks: the route (every refusal comes before the iters == 0 return), then B staged once
// per call and only when there are iterations to run, then the engine.
static int run_lockstep(const LockstepCall& c) {
  LockstepRoute r;
  if (int rc = lockstep_route(c, &r)) return rc;
  if (c.iters == 0) return FOS_OK;
  if (r.engine == ENGINE_SINGLE) return fos_fista_run(c.fs[0], c.iters);
  if (r.stage_b)
    if (int rc = stage_b16(c.fs[0]->p, c.B, c.ldb, c.nv)) return rc;
  return r.engine == ENGINE_VALU ? run_multi_valu(c, r) : run_multi_mfma(c, r);
}

int fos_fista_run_multi(fos_fista* const* fs, int nv, int iters) {
  if (!fs || nv < 1 || nv > fos::BT_NV || iters < 0) return fail(FOS_ERR_ARG, "fos_fista_run_multi: bad argument");
  for (int v = 0; v < nv; ++v)
    if (!fs[v] || fs[v]->p != fs[0]->p) return fail(FOS_ERR_ARG, "fos_fista_run_multi: handles must share one problem");
  return run_lockstep(LockstepCall{fs, nv, iters, nullptr, 0, nullptr, nullptr, nullptr, "fos_fista_run_multi"});
}

int fos_fista_run_multi_rhs(fos_fista* const* fs, int nv, const float* B, int64_t ldb, int iters) {
  if (!fs || !B || nv < 1 || nv > fos::BT_NV || ldb < nv || iters < 0)
    return fail(FOS_ERR_ARG, "fos_fista_run_multi_rhs: bad argument (null pointer, nv outside 1..16, ldb < nv or iters < 0)");
  for (int v = 0; v < nv; ++v)
    if (!fs[v] || fs[v]->p != fs[0]->p) return fail(FOS_ERR_ARG, "fos_fista_run_multi_rhs: handles must share one problem");
  if (int rc_ = group_takes_block(fs, nv) ? FOS_OK : need_squared(fs[0]->p, "fos_fista_run_multi_rhs")) return rc_;
  return run_lockstep(LockstepCall{fs, nv, iters, B, ldb, nullptr, nullptr, nullptr, "fos_fista_run_multi_rhs"});
}

int fos_fista_run_multi_folds(fos_fista* const* fs, int nv, int iters, const uint8_t* fold_of_row, const int32_t* held) {
  fos::FoldHeld hb{};
  if (!fs || !fold_of_row || !held || nv < 1 || nv > fos::BT_NV || iters < 0 || ((uintptr_t)fold_of_row & 3) != 0 ||
      !fold_held_block(held, nv, &hb))
    return fail(FOS_ERR_ARG, "fos_fista_run_multi_folds: bad argument (null pointer, nv outside 1..16, iters < 0, fold_of_row "
                             "not 4-byte aligned or a held id outside -1..254)");
  for (int v = 0; v < nv; ++v)
    if (!fs[v] || fs[v]->p != fs[0]->p) return fail(FOS_ERR_ARG, "fos_fista_run_multi_folds: handles must share one problem");
  return run_lockstep(LockstepCall{fs, nv, iters, nullptr, 0, fold_of_row, held, &hb, "fos_fista_run_multi_folds"});
}

// What a resampled pass (include/fos_resample.h) does not serve, in its own words and before any launch or change of handle
// state: the link kernel needs whole columns that are fits of their own, b, one card and the matrix-core pair.  needs_b: null for
// the loss-free operator.
static int resample_refusal(const fos_problem* p, const char* fn, const char* needs_b) {
  if (p->loss == FOS_LOSS_MULTINOMIAL)
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": a multinomial problem is not served: its columns are the classes of joint "
                                     "fits, not fits of their own (squared, logistic, Huber and squared-hinge loss)");
  if (needs_b && !p->b) return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": " + needs_b);
  if (p->comm || p->col_sharded)
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": row- or column-sharded problems are not served (the counts are those of all rows)");
  if (!pair_dd_multi_supported(p)) return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": the shape has no matrix-core pair");
  return FOS_OK;
}

// (include/fos_resample.h declares it, not fos.h: the linkage is spelled out here, as on no entry point of fos.h's closed list)
extern "C" int fos_fista_run_multi_resampled(fos_fista* const* fs, int nv, int iters, const uint64_t* counts) {
  const char* fn = "fos_fista_run_multi_resampled";
  if (!fs || !counts || nv < 1 || nv > fos::BT_NV || iters < 0 || ((uintptr_t)counts & 7) != 0)
    return fail(FOS_ERR_ARG, std::string(fn) + ": bad argument (null pointer, nv outside 1..16, iters < 0 or counts not 8-byte aligned)");
  for (int v = 0; v < nv; ++v)
    if (!fs[v] || fs[v]->p != fs[0]->p) return fail(FOS_ERR_ARG, std::string(fn) + ": handles must share one problem");
  if (int rc_ = resample_refusal(fs[0]->p, fn, "the resampled data term needs b")) return rc_;
  for (int v = 0; v < nv; ++v) {
    if (grouped(fs[v]->prm))
      return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": the group penalty across columns (fos_fista_params.group >= 2) ties the "
                                       "columns into one fit; a resample per column would break it");
    if (fs[v]->prm.tol_grad != 0.0 || fs[v]->precise || fs[v]->prm.tau_from_state)
      return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": no gradient-norm rule, fp64 split gradient or device-held step (plain "
                                       "runs, adaptive restart, step and ratio tolerance per column)");
  }
  return run_lockstep(LockstepCall{fs, nv, iters, nullptr, 0, nullptr, nullptr, nullptr, fn, counts});
}

// G[j][c] = sum over the row splits of slabs16[split][j][c]: the slab sum of fos_gram_apply.
static __global__ __launch_bounds__(256) void gram_slab_sum_kernel(const float* __restrict__ slabs, int splits, int64_t n, int nv,
                                                                   float* __restrict__ G) {
  const int64_t total = (int64_t)nv * n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    float acc = 0.f;                 // i = j * n + c; a slab set is 16 x n floats
    for (int s = 0; s < splits; ++s) acc += slabs[(int64_t)s * fos::BT_NV * n + i];
    G[i] = acc;
  }
}

int fos_gram_apply(const float* X, int nv, fos_problem* p, float* G) {
  if (!X || !p || !G || nv < 1 || nv > fos::BT_NV) return fail(FOS_ERR_ARG, "fos_gram_apply: bad argument (null pointer or nv outside 1..16)");
  if (!pair_dd_multi_supported(p)) return fail(FOS_ERR_UNSUPPORTED, "fos_gram_apply: the shape has no matrix-core pair");
  int rc = ensure_batch_workspace(p);
  if (rc) return rc;
  if ((rc = plan_multi_mfma(p))) return rc;
  int g_splits = 0;
  if ((rc = two_product_splits(p, &g_splits))) return rc;
  const int64_t esz = p->dtype == FOS_BF16 ? 2 : 4;
  if ((rc = pack_candidates(p, X, nv))) return rc;
  for (int64_t row0 = 0, panel = 0; row0 < p->m; row0 += p->multi.panel_rows, ++panel) {
    const int64_t rows = std::min<int64_t>(p->multi.panel_rows, p->m - row0);
    const char* Ap = reinterpret_cast<const char*>(p->A) + (size_t)row0 * p->lda * esz;
    int nwg1 = 0;
    BatchLaunch L{};                 // R = A_panel X, or w (A_panel X): neither b nor the loss enters
    L.A = Ap; L.rows = rows; L.rout = p->multi.rbuf16; L.row_weight = p->row_weight ? p->row_weight + row0 : nullptr;
    if ((rc = launch_batch_product(p, L, &nwg1))) return rc;
    if ((rc = launch_gram_panel(p, Ap, rows, g_splits, panel != 0))) return rc;
  }
  hipLaunchKernelGGL(gram_slab_sum_kernel, dim3(grid_1d((int64_t)nv * p->n, 256, 1024)), dim3(256), 0, p->stream, p->multi.slabs16,
                     g_splits, p->n, nv, G);
  LAUNCH_CHECK();
  return FOS_OK;
}

// fos_gram_apply with a resample per column: product 1 plain, the Gram form of the resample link kernel - R = (w c_j) z, the
// bound weights enter there -, product 2.
int fos_gram_apply_resampled(const float* X, int nv, const uint64_t* counts, fos_problem* p, float* G) {
  if (!X || !counts || !p || !G || nv < 1 || nv > fos::BT_NV || ((uintptr_t)counts & 7) != 0)
    return fail(FOS_ERR_ARG, "fos_gram_apply_resampled: bad argument (null pointer, nv outside 1..16 or counts not 8-byte aligned)");
  int rc = resample_refusal(p, "fos_gram_apply_resampled", nullptr);
  if (rc) return rc;
  if ((rc = ensure_batch_workspace(p))) return rc;
  if ((rc = plan_multi_mfma(p))) return rc;
  int g_splits = 0;
  if ((rc = two_product_splits(p, &g_splits))) return rc;
  const int64_t esz = p->dtype == FOS_BF16 ? 2 : 4;
  if ((rc = pack_candidates(p, X, nv))) return rc;
  for (int64_t row0 = 0, panel = 0; row0 < p->m; row0 += p->multi.panel_rows, ++panel) {
    const int64_t rows = std::min<int64_t>(p->multi.panel_rows, p->m - row0);
    const char* Ap = reinterpret_cast<const char*>(p->A) + (size_t)row0 * p->lda * esz;
    int nwg1 = 0;
    BatchLaunch L{};                 // Z = A_panel X
    L.A = Ap; L.rows = rows; L.rout = p->multi.rbuf16;
    if ((rc = launch_batch_product(p, L, &nwg1))) return rc;
    if ((rc = launch_resample_link(p, true, row0, rows, nv, counts, 0, nullptr, &nwg1))) return rc;
    if ((rc = launch_gram_panel(p, Ap, rows, g_splits, panel != 0))) return rc;
  }
  hipLaunchKernelGGL(gram_slab_sum_kernel, dim3(grid_1d((int64_t)nv * p->n, 256, 1024)), dim3(256), 0, p->stream, p->multi.slabs16,
                     g_splits, p->n, nv, G);
  LAUNCH_CHECK();
  return FOS_OK;
}

int fos_fista_grad(fos_fista* f) {
  if (!f) return fail(FOS_ERR_ARG, "fos_fista_grad: null");
  if (int rc_ = need_squared(f->p, "fos_fista_grad")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_grad")) return rc_;
  fos_problem* p = f->p;
  int n_rr = 0, rc;
  if (f->precise && !p->pass.resident) {
    // fp64-accumulating pass at the unrounded y_k = x_k + beta (x_k - x_{k-1}); alpha2*y is added by the consumers
    YSource ys = (plain_run(f) && f->host_valid)
                     ? YSource{nullptr, f->x_cur, f->x_prev, nullptr, &f->scal->stopped, f->h_beta, nullptr}
                     : fista_source(f);
    if ((rc = launch_pass_dd(p, ys, 0.0, nullptr, f->gbuf64))) return rc;
    hipLaunchKernelGGL(rr_from_gbuf64_kernel, dim3(1), dim3(1), 0, p->stream, f->gbuf64, (int)p->n, &f->scal->rr,
                       &f->scal->stopped);
    LAUNCH_CHECK();
    return FOS_OK;
  }
  const YSource ys = (plain_run(f) && f->host_valid && !p->col_sharded) ? plain_source(f) : fista_source(f);
  if ((rc = launch_pass(p, ys, p->b, true, &n_rr))) return rc;
  return launch_slab_reduce(p, n_rr, p->gbuf, &f->scal->rr, &f->scal->stopped);
}

int fos_fista_grad_dual(fos_fista* f) {
  if (!f) return fail(FOS_ERR_ARG, "fos_fista_grad_dual: null");
  if (int rc_ = need_squared(f->p, "fos_fista_grad_dual")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_grad_dual")) return rc_;
  fos_problem* p = f->p;
  int n_rr = 0, rc;
  if ((rc = flush_pending(f))) return rc;
  if (p->pass.path == 0 && !p->pass.colblock && p->pass.entry->dual != nullptr && !(f->precise && !p->pass.resident)) {
    if ((rc = launch_pass(p, fista_source(f), p->b, true, &n_rr, true))) return rc;
    if ((rc = launch_slab_reduce(p, n_rr, p->gbuf, &f->scal->rr, &f->scal->stopped))) return rc;
    hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, p->pass.rr2_part, n_rr, 1,
                       &f->scal->rr_x);
    LAUNCH_CHECK();
    return p->col_sharded ? FOS_OK : reduce_across(p, &f->scal->rr_x, 1, true);
  }
  // no DUAL instantiation (fallback path / wide geometries): a separate residual pass on x_k, then the gradient
  hipLaunchKernelGGL(fos::cast_f64_f32_kernel, dim3(grid_1d(p->n, 256, 1024)), dim3(256), 0, p->stream, f->x_cur, p->ws.ybuf,
                     p->n);
  LAUNCH_CHECK();
  YSource ys{p->ws.ybuf, nullptr, nullptr, nullptr, &f->scal->stopped};
  if ((rc = launch_pass(p, ys, p->b, false, &n_rr))) return rc;
  hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, p->pass.rr_part, n_rr, 1,
                     &f->scal->rr_x);
  LAUNCH_CHECK();
  if (!p->col_sharded && (rc = reduce_across(p, &f->scal->rr_x, 1, true))) return rc;
  return fos_fista_grad(f);
}

int fos_fista_update(fos_fista* f) {
  if (!f) return fail(FOS_ERR_ARG, "fos_fista_update: null");
  if (int rc_ = need_squared(f->p, "fos_fista_update")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_update")) return rc_;
  fos_problem* p = f->p;
  if (plain_run(f) && f->host_valid && !p->col_sharded) {
    // host-driven momentum (see fos_fista_run): no per-iteration bookkeeping launch, y handed on as one fp32 vector
    const PlainStep s = advance_plain(f, true);
    return launch_update(f, nullptr, 0, grad_src(f), f->prm, s.part, 1, s.beta, nullptr, f->ynext, s.beta_next);
  }
  hand_to_device(f);
  int rc = launch_update(f, nullptr, 0, grad_src(f), f->prm, p->ws.part, 0, 0.0, nullptr, nullptr, 0.0);
  return rc ? rc : launch_finalize(f, 0);
}

int fos_fista_trial(fos_fista* f, double t, int with_residual, double out8[8]) {
  if (!f || !out8 || !(t > 0.0)) return fail(FOS_ERR_ARG, "fos_fista_trial: bad argument");
  if (int rc_ = need_squared(f->p, "fos_fista_trial")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_trial")) return rc_;
  fos_problem* p = f->p;
  if (p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, "fos_fista_trial: no column-sharded form (||A dlt||^2 needs an m-vector exchange per candidate)");
  { int rcf = flush_pending(f); if (rcf) return rcf; }
  const int grid = grid_1d(p->n, 256, 256);
  HIP_TRY(hipMemsetAsync(f->out5, 0, 8 * sizeof(double), p->stream));
  hipLaunchKernelGGL(fos::fista_trial_kernel, dim3(grid), dim3(256), 0, p->stream, grad_src(f), (int)p->n, f->x_cur,
                     f->x_prev, f->scal, f->prm, t, f->dlt, p->ws.part);
  hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, p->ws.part, grid, fos::TRIAL_W, f->out5);
  LAUNCH_CHECK();
  // rr(y_k) was produced by fos_fista_grad; copy it before the trial pass reuses the partial buffer
  HIP_TRY(hipMemcpyAsync(f->out5 + 6, &f->scal->rr, sizeof(double), hipMemcpyDeviceToDevice, p->stream));
  if (with_residual) {
    YSource ys{f->dlt, nullptr, nullptr, nullptr, nullptr};
    int n_rr = 0, rc;
    if ((rc = launch_pass(p, ys, nullptr, false, &n_rr))) return rc;        // ||A dlt||^2  (b = 0)
    hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, p->pass.rr_part, n_rr, 1, f->out5 + 5);
    LAUNCH_CHECK();
    if ((rc = reduce_across(p, f->out5 + 5, 1, true))) return rc;
  }
  HIP_TRY(hipMemcpyAsync(out8, f->out5, 8 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return FOS_OK;
}

// Enqueue one batch of Armijo candidates t, t*eta, ...: candidate kernel, fold of its sums -> bt_out[0..50), the matrix-
// core pass ||A dlt_j||^2 -> bt_out[64..80).  t_from_state: t is FistaScalars::tau on the device (no host value).
static int enqueue_trial_batch(fos_fista* f, double t, double eta, int nv, int t_from_state) {
  fos_problem* p = f->p;
  const int grid = grid_1d(p->cand.n_pad, 256, 64);
  const int* stopped = t_from_state ? &f->scal->stopped : nullptr;
  if (p->dtype == FOS_BF16)
    hipLaunchKernelGGL(fos::fista_trial_batch_bf16_kernel, dim3(grid), dim3(256), 0, p->stream, grad_src(f), (int)p->n,
                       (int)p->cand.n_pad, f->x_cur, f->x_prev, f->scal, f->prm, t, eta, nv, (unsigned short*)p->cand.xp.get(), p->ws.part,
                       t_from_state);
  else
    hipLaunchKernelGGL(fos::fista_trial_batch_kernel, dim3(grid), dim3(256), 0, p->stream, grad_src(f), (int)p->n,
                       (int)p->cand.n_pad, f->x_cur, f->x_prev, f->scal, f->prm, t, eta, nv, p->cand.xp, p->ws.part, t_from_state);
  hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, p->ws.part, grid, fos::BT_W, p->cand.bt_out);
  LAUNCH_CHECK();
  if (p->col_sharded) {              // grad.dlt_j, ||dlt_j||^2, the counts, ||grad||^2, ||y||^2 are sums over the column blocks
    int rc = reduce_across(p, p->cand.bt_out, fos::BT_W, true);
    if (rc) return rc;
  }
  return launch_residual_batch(p, 0, p->cand.bt_out + 64, stopped);
}

// Device-driven iterations with data-dependent control - Armijo search, adaptive restart, the stopping rules - and,
// optionally, the history recorded on the device.  One body behind fos_fista_run_backtracking and fos_fista_run_recorded.
static int run_device_driven(fos_fista* f, int iters, bool backtracking, double eta, double armijo_c, double grad_eps,
                             int32_t* ls_iters, double* tau_hist, double* x_hist, double* hist, double* rr_seen) {
  fos_problem* p = f->p;
  int rc = flush_pending(f);
  if (rc) return rc;
  if ((rc = ensure_packed(p))) return rc;
  if (backtracking) {
    if ((rc = ensure_batch_workspace(p))) return rc;
    // the step lives on the device from here on (tau persists, :197)
    if (!f->tau_on_device) {
      hipLaunchKernelGGL(fos::set_state_tau_kernel, dim3(1), dim3(1), 0, p->stream, f->scal, f->prm.tau);
      LAUNCH_CHECK();
      f->tau_on_device = true;
    }
  }
  hand_to_device(f);
  fos::FistaParams prm_dev = f->prm;
  prm_dev.tau_from_state = backtracking ? 1 : 0;
  const bool record = hist != nullptr;
  for (int it = 0; it < iters; ++it) {
    // gradient (:173-175; the fp64 pass in precise mode); recording: the same pass (or a residual pass of its own where
    // there is no DUAL kernel) also yields ||A x_k - b||^2 of the iterate this iteration starts from
    if (record && rr_seen != nullptr) {
      if ((rc = fos_fista_grad_dual(f))) return rc;
      hipLaunchKernelGGL(fos::record_rr_x_kernel, dim3(1), dim3(1), 0, p->stream, f->scal, rr_seen + it);
      LAUNCH_CHECK();
    } else if ((rc = fos_fista_grad(f))) {
      return rc;
    }
    if (f->prm.tol_grad > 0.0 && (rc = launch_grad_norm_stop(f))) return rc;   // :179
    if (backtracking) {
      if ((rc = enqueue_trial_batch(f, 0.0, eta, fos::BT_NV, 1))) return rc;   // :187-191 for 16 candidates
      hipLaunchKernelGGL(fos::armijo_decide_kernel, dim3(1), dim3(1), 0, p->stream, p->cand.bt_out, f->scal, f->prm, eta,
                         armijo_c, grad_eps, fos::BT_NV, ls_iters, tau_hist, (long long)it);
      LAUNCH_CHECK();
    }
    // update (with the step the decision left in FistaScalars::tau), then the scalar bookkeeping / history row
    double* xrow = x_hist ? x_hist + (size_t)it * p->n : nullptr;
    if ((rc = launch_update(f, nullptr, 0, grad_src(f), prm_dev, p->ws.part, 0, 0.0, xrow, nullptr, 0.0))) return rc;
    if ((rc = launch_finalize(f, 0, record ? hist + (size_t)it * 4 : nullptr))) return rc;
  }
  return FOS_OK;
}

int fos_fista_run_backtracking(fos_fista* f, int iters, double eta, double armijo_c, double grad_eps, int32_t* ls_iters,
                               double* tau_hist) {
  if (!f || iters < 0 || !(eta > 0.0 && eta < 1.0) || !(grad_eps >= 0.0))
    return fail(FOS_ERR_ARG, "fos_fista_run_backtracking: bad argument");
  if (int rc_ = need_squared(f->p, "fos_fista_run_backtracking")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_run_backtracking")) return rc_;
  fos_problem* p = f->p;
  if (!batch_supported(p) || p->pass.resident)
    return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_backtracking: needs the matrix-core candidate pass (streaming plans)");
  if (iters == 0) return FOS_OK;
  return run_device_driven(f, iters, true, eta, armijo_c, grad_eps, ls_iters, tau_hist, nullptr, nullptr, nullptr);
}

int fos_fista_run_recorded(fos_fista* f, int iters, int backtracking, double eta, double armijo_c, double grad_eps,
                           double* x_hist, double* hist, double* rr_seen, int32_t* ls_iters, double* tau_hist) {
  if (!f || iters < 0 || (iters > 0 && (!x_hist || !hist)) ||
      (backtracking && (!(eta > 0.0 && eta < 1.0) || !(grad_eps >= 0.0))))
    return fail(FOS_ERR_ARG, "fos_fista_run_recorded: bad argument");
  if (int rc_ = need_squared(f->p, "fos_fista_run_recorded")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_run_recorded")) return rc_;
  fos_problem* p = f->p;
  if (p->pass.resident || (backtracking && !batch_supported(p)))
    return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_recorded: resident problems record inside their one launch; "
                                     "backtracking needs the matrix-core candidate pass");
  if (iters == 0) return FOS_OK;
  return run_device_driven(f, iters, backtracking != 0, eta, armijo_c, grad_eps, ls_iters, tau_hist, x_hist, hist, rr_seen);
}

int fos_fista_resume_after_stall(fos_fista* f, double* tau_out) {
  if (!f || !tau_out) return fail(FOS_ERR_ARG, "fos_fista_resume_after_stall: null");
  if (int rc_ = need_squared(f->p, "fos_fista_resume_after_stall")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_resume_after_stall")) return rc_;
  fos_problem* p = f->p;
  fos::FistaScalars h;
  HIP_TRY(hipMemcpyAsync(&h, f->scal, sizeof(h), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  *tau_out = h.tau;
  f->prm.tau = h.tau;                          // tau persists (:197), also across the hand-over to the host
  hipLaunchKernelGGL(fos::clear_stall_kernel, dim3(1), dim3(1), 0, p->stream, f->scal);
  LAUNCH_CHECK();
  return FOS_OK;
}

int fos_fista_trial_batch(fos_fista* f, double t, double eta, int nv, double* out) {
  if (!f || !out || !(t > 0.0) || !(eta > 0.0) || nv < 1 || nv > fos::BT_NV)
    return fail(FOS_ERR_ARG, "fos_fista_trial_batch: bad argument");
  if (int rc_ = need_squared(f->p, "fos_fista_trial_batch")) return rc_;
  if (int rc_ = need_separable(f, "fos_fista_trial_batch")) return rc_;
  fos_problem* p = f->p;
  { int rcf = flush_pending(f); if (rcf) return rcf; }
  if (!batch_supported(p)) return fail(FOS_ERR_UNSUPPORTED, "fos_fista_trial_batch: needs the fused path");
  int rc = ensure_batch_workspace(p);
  if (rc) return rc;
  if ((rc = enqueue_trial_batch(f, t, eta, nv, 0))) return rc;
  HIP_TRY(hipMemcpyAsync(p->cand.bt_out + 100, &f->scal->rr, sizeof(double), hipMemcpyDeviceToDevice, p->stream));
  double h[128];
  HIP_TRY(hipMemcpyAsync(h, p->cand.bt_out, 128 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  for (int j = 0; j < nv; ++j) {
    double* o = out + 8 * j;
    o[0] = h[j];                        // grad . dlt_j
    o[1] = h[fos::BT_NV + j];           // ||dlt_j||^2
    o[2] = h[2 * fos::BT_NV + j];       // #(dlt_j != 0)
    o[3] = h[3 * fos::BT_NV];           // ||grad||^2
    o[4] = h[3 * fos::BT_NV + 1];       // ||y||^2
    o[5] = h[64 + j];                   // ||A dlt_j||^2
    o[6] = h[100];                      // ||A y - b||^2
    o[7] = 0.0;
  }
  return FOS_OK;
}

int fos_fista_status_get(fos_fista* f, fos_fista_status* out) {
  if (!f || !out) return fail(FOS_ERR_ARG, "fos_fista_status_get: null");
  { int rcf = flush_pending(f); if (rcf) return rcf; }
  fos::FistaScalars h;
  HIP_TRY(hipMemcpyAsync(&h, f->scal, sizeof(h), hipMemcpyDeviceToHost, f->p->stream));
  HIP_TRY(hipStreamSynchronize(f->p->stream));
  out->t_prev = h.t_prev; out->beta = h.beta; out->this_step = h.this_step; out->prev_step = h.prev_step;
  out->ratio = h.ratio; out->rr = h.rr; out->gnorm2 = h.gnorm2; out->xnorm1 = h.xnorm1; out->xnorm2 = h.xnorm2;
  out->rr_x = h.rr_x;
  out->tau = h.tau;
  out->k = h.k; out->stopped = h.stopped; out->restarts = h.restarts;
  return FOS_OK;
}

int fos_fista_get_x(fos_fista* f, double* dst) {
  if (!f || !dst) return fail(FOS_ERR_ARG, "fos_fista_get_x: null");
  HIP_TRY(hipMemcpyAsync(dst, f->x_cur, (size_t)f->p->n * sizeof(double), hipMemcpyDeviceToDevice, f->p->stream));
  return FOS_OK;
}
double* fos_fista_x(fos_fista* f) { return f ? f->x_cur : nullptr; }
float* fos_fista_gbuf(fos_fista* f) { return f ? f->p->gbuf : nullptr; }

// ---- batches of small problems: one workgroup per problem, one launch per SMALL class (resident_batch.hpp) ----------
int64_t fos_fista_batch_workspace(int count, int64_t ldx) {
  if (count < 0 || ldx < 1) return -1;
  return (int64_t)count * ((int64_t)sizeof(fos::ResidentBatchDesc) + (int64_t)sizeof(fos::FistaScalars) +
                           ldx * (int64_t)sizeof(double));
}

int fos_fista_run_batch(const void* A, int a_dtype, const float* b, const fos_batch_item* items, const fos_fista_params* prm,
                        int count, int iters, int backtracking, double eta, double armijo_c, int64_t ldx, double* x_out,
                        int32_t* iters_done, int32_t* stopped, double* tau_out, int32_t* ls_iters, double* tau_hist,
                        double* hist, double* x_hist, void* work, void* stream) {
  if (count < 0 || iters < 0 || (backtracking && !(eta > 0.0 && eta < 1.0)) || (a_dtype != FOS_F32 && a_dtype != FOS_BF16))
    return fail(FOS_ERR_ARG, "fos_fista_run_batch: bad argument (count < 0, iters < 0, eta outside (0, 1) or a_dtype)");
  if (count == 0) return FOS_OK;
  if (!A || !b || !items || !prm || !x_out || !iters_done || !stopped || !tau_out || !work || ldx < 1)
    return fail(FOS_ERR_ARG, "fos_fista_run_batch: bad argument (null pointer or ldx < 1)");
  if (int rc = check_batch_items("fos_fista_run_batch", items, count, ldx)) return rc;
  int n_small = 0;
  for (int i = 0; i < count; ++i) {
    const fos_fista_params& q = prm[i];
    if (q.mode < 0 || q.mode > 2 || q.prox_kind < 0 || q.prox_kind > 1 || !(q.tau > 0.0) || q.tol_grad < 0.0 ||
        q.tol_step < 0.0 || q.tol_ratio < 0.0)
      return fail(FOS_ERR_ARG, "fos_fista_run_batch: bad argument (prm " + std::to_string(i) +
                                   ": mode / prox_kind / tau / tolerance)");
    if (q.group < 0 || q.group > fos::BT_NV)
      return fail(FOS_ERR_ARG, "fos_fista_run_batch: bad argument (prm " + std::to_string(i) + ": group outside 0..16)");
    if (q.group >= 2)
      return fail(FOS_ERR_UNSUPPORTED, "fos_fista_run_batch: the group penalty (fos_fista_params.group >= 2) couples lockstep "
                                       "columns; a batch member is a problem of its own");
    n_small += items[i].n <= fos::RS_CHUNK && items[i].m <= fos::RS_SMALL_M;
  }
  // SMALL problems (rows of A in registers: run_resident's rule) at [0, n_small), the others after them, each class one
  // launch over its own range
  std::vector<fos::ResidentBatchDesc> d(count);
  for (int i = 0, s = 0, l = n_small; i < count; ++i) {
    const fos_batch_item& it = items[i];
    fos::ResidentBatchDesc& e = d[it.n <= fos::RS_CHUNK && it.m <= fos::RS_SMALL_M ? s++ : l++];
    e.a_offset = it.a_offset;
    e.lda = it.lda;
    e.b_offset = it.b_offset;
    e.m = it.m;
    e.n = it.n;
    e.idx = i;
    e.pad_ = 0;
    to_dev_params(&prm[i], &e.prm);
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  auto* desc = reinterpret_cast<fos::ResidentBatchDesc*>(work);
  fos::ResidentBatchOut o{};
  o.ldx = ldx;
  o.x_out = x_out;
  o.iters_done = iters_done;
  o.stopped = stopped;
  o.tau_final = tau_out;
  o.ls_out = ls_iters;
  o.tau_out = tau_hist;
  o.hist = hist;
  o.x_hist = x_hist;
  o.scal = reinterpret_cast<fos::FistaScalars*>(desc + count);
  o.x_prev = reinterpret_cast<double*>(o.scal + count);
  HIP_TRY(hipMemcpyAsync(desc, d.data(), (size_t)count * sizeof(fos::ResidentBatchDesc), hipMemcpyHostToDevice, st));
#define FOS_RSB_LAUNCH(T, SMALL, G, D)                                                                                   \
  hipLaunchKernelGGL((fos::fista_resident_batch_kernel<T, SMALL>), dim3(G), dim3(fos::RS_THREADS), 0, st,               \
                     (const T*)A, b, D, iters, backtracking ? 1 : 0, eta, armijo_c, o)
  const int n_large = count - n_small;
  if (a_dtype == FOS_F32) {
    if (n_small) FOS_RSB_LAUNCH(float, true, n_small, desc);
    if (n_large) FOS_RSB_LAUNCH(float, false, n_large, desc + n_small);
  } else {
    if (n_small) FOS_RSB_LAUNCH(fos::bf16_t, true, n_small, desc);
    if (n_large) FOS_RSB_LAUNCH(fos::bf16_t, false, n_large, desc + n_small);
  }
#undef FOS_RSB_LAUNCH
  LAUNCH_CHECK();
  return FOS_OK;
}

}  // extern "C"

// ---- Working-set solve and duality-gap certificate of every loss family (include/fos_working_set.h, fos_duality.h,
// fos_multinomial_ws.h; working_set.hpp, duality.hpp, multinomial_ws.hpp) -------------------------------------------------------
// The shapes the two-product walks serve: b (or the labels) bound, one card, the matrix-core pair.  needs_b: the caller's words
// for a problem without b.
static int need_two_products(const fos_problem* p, const std::string& fn, const char* needs_b) {
  if (!p->b) return fail(FOS_ERR_UNSUPPORTED, fn + ": " + needs_b);
  if (p->comm || p->col_sharded) return fail(FOS_ERR_UNSUPPORTED, fn + ": sharded problems are not served");
  if (!pair_dd_multi_supported(p)) return fail(FOS_ERR_UNSUPPORTED, fn + ": the shape has no matrix-core pair");
  return FOS_OK;
}

// The checks the three multinomial entry points share, after their own FOS_ERR_ARG rows: a multinomial problem whose class
// count divides nv.
static int need_class_segments(const fos_problem* p, int nv, const char* fn) {
  if (p->loss != FOS_LOSS_MULTINOMIAL)
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": the problem is not multinomial (fos_gradient_batch, fos_kkt_scan and "
                                     "fos_duality_gap serve the other losses)");
  if (p->classes < 2 || nv % p->classes != 0)
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": nv is not a multiple of the " + std::to_string(p->classes) + " classes");
  return FOS_OK;
}

// The per-fit weights of a call (HOST memory, nfits each: nv, or nv / C on a multinomial problem; a2 may be null), checked:
// FOS_ERR_ARG before any HIP call.
static int class_weights(int nfits, const double* a1, const double* a2, const char* fn, fos::ClassWeights* w) {
  *w = fos::ClassWeights{};
  for (int s = 0; s < nfits; ++s) {
    if (!(std::isfinite(a1[s]) && a1[s] >= 0.0) || (a2 && !(std::isfinite(a2[s]) && a2[s] >= 0.0)))
      return fail(FOS_ERR_ARG, std::string(fn) + ": weight " + std::to_string(s) + " is not finite and >= 0");
    w->a1[s] = a1[s];
    w->a2[s] = a2 ? a2[s] : 0.0;
  }
  return FOS_OK;
}

// What a loss family puts between product 1 and product 2 of the gradient walk.
enum class WalkLink { none, pointwise, softmax, resample };
struct GradientWalk {
  const char* fn;        // the entry point, for the messages
  const char* needs_b;   // its words for a problem without b
  bool plain;            // product 1 without b and the bound weights (Z = A_panel X: a link kernel follows); else with them
  WalkLink link;         // none: product 1's own loss epilogue; launch_pointwise_link; launch_softmax_link; launch_resample_link
  bool staged;           // the panel's partials land in cand.q_part (several panels: copied behind each other into
                         // ws.grad_part); else behind those of the panels before it in ws.link_part
  const uint64_t* counts = nullptr;      // WalkLink::resample: the multiplicity words of all rows
  int oob = 0;           // ... and whether only the out-of-bag sums are wanted: product 2 and the slab sum do not run, G is not written
};

// The gradient of the data term at the nv columns of X: per row panel product 1 in its storing form, the family's link stage and
// product 2, then the slab sum of fos_gram_apply and, for loss16, one fold of the loss partials of all panels.
static int gradient_walk(const GradientWalk& w, const float* X, int nv, fos_problem* p, float* G, double* loss16) {
  int rc = need_two_products(p, w.fn, w.needs_b);
  if (rc) return rc;
  if ((rc = ensure_batch_workspace(p))) return rc;
  if ((rc = plan_multi_mfma(p))) return rc;
  int g_splits = 0;
  if ((rc = two_product_splits(p, &g_splits))) return rc;
  const int64_t panels = (p->m + p->multi.panel_rows - 1) / p->multi.panel_rows;
  const size_t part_rows = (size_t)(3 * p->ncu + 8);               // the rows of cand.q_part
  const bool copied = w.staged && loss16 && panels > 1;
  if (copied && (rc = p->ws.grad_part.reserve((size_t)panels * part_rows * fos::BT_NV))) return rc;
  if (!w.staged && (rc = p->ws.link_part.reserve((size_t)panels * p->ncu * fos::BT_NV))) return rc;
  const int64_t esz = p->dtype == FOS_BF16 ? 2 : 4;
  if ((rc = pack_candidates(p, X, nv))) return rc;
  int nparts = 0;
  for (int64_t row0 = 0, panel = 0; row0 < p->m; row0 += p->multi.panel_rows, ++panel) {
    const int64_t rows = std::min<int64_t>(p->multi.panel_rows, p->m - row0);
    const char* Ap = reinterpret_cast<const char*>(p->A) + (size_t)row0 * p->lda * esz;
    int nwg = 0;
    BatchLaunch L{};                 // plain: Z = A_panel X; else R = w (A_panel X - b) or w (sigma(A_panel X) - b)
    L.A = Ap; L.rows = rows; L.rout = p->multi.rbuf16;
    if (!w.plain) {                  // labels and weights are offset with the panel
      L.b = p->b + row0; L.use_b = 1;
      L.row_weight = p->row_weight ? p->row_weight + row0 : nullptr;
    }
    if ((rc = launch_batch_product(p, L, &nwg))) return rc;
    double* part = w.staged ? p->cand.q_part.get() : p->ws.link_part + (size_t)nparts * fos::BT_NV;
    if (w.link == WalkLink::pointwise && (rc = launch_pointwise_link(p, row0, rows, nv, fos::FOLD_OFF, nullptr, nullptr, part, &nwg))) return rc;
    if (w.link == WalkLink::softmax && (rc = launch_softmax_link(p, row0, rows, nv, fos::FOLD_OFF, nullptr, nullptr, part, &nwg))) return rc;
    if (w.link == WalkLink::resample && (rc = launch_resample_link(p, false, row0, rows, nv, w.counts, w.oob, part, &nwg))) return rc;
    if (copied) {
      if ((size_t)nwg > part_rows) return fail(FOS_ERR_STATE, std::string(w.fn) + ": product 1 wrote more partials than cand.q_part holds");
      HIP_TRY(hipMemcpyAsync(p->ws.grad_part + (size_t)nparts * fos::BT_NV, part, (size_t)nwg * fos::BT_NV * sizeof(double),
                             hipMemcpyDeviceToDevice, p->stream));
    }
    nparts += nwg;
    if (!w.oob && (rc = launch_gram_panel(p, Ap, rows, g_splits, panel != 0))) return rc;
  }
  if (!w.oob) {
    hipLaunchKernelGGL(gram_slab_sum_kernel, dim3(grid_1d((int64_t)nv * p->n, 256, 1024)), dim3(256), 0, p->stream, p->multi.slabs16,
                       g_splits, p->n, nv, G);
    LAUNCH_CHECK();
  }
  if (loss16) {
    const double* parts = !w.staged ? p->ws.link_part.get() : copied ? p->ws.grad_part.get() : p->cand.q_part.get();
    hipLaunchKernelGGL(fos::fold_partials_kernel, dim3(1), dim3(fos::FOLD_THREADS), 0, p->stream, parts, nparts, fos::BT_NV, loss16);
    LAUNCH_CHECK();
  }
  return FOS_OK;
}

extern "C" {

// Product 1 runs with b, the problem's loss epilogue and the bound weights and leaves the loss partials itself; on a Huber or
// squared-hinge problem it runs plain and the pointwise link kernel leaves R and the partials instead.
int fos_gradient_batch(const float* X, int nv, fos_problem* p, float* G, double* loss16) {
  if (!X || !p || !G || nv < 1 || nv > fos::BT_NV)
    return fail(FOS_ERR_ARG, "fos_gradient_batch: bad argument (null pointer or nv outside 1..16)");
  if (p->loss == FOS_LOSS_MULTINOMIAL)
    return fail(FOS_ERR_UNSUPPORTED, "fos_gradient_batch: a multinomial problem is not served (squared and logistic loss)");
  const bool link = link_loss(p);
  return gradient_walk({"fos_gradient_batch", "the gradient of the data term needs b", link, link ? WalkLink::pointwise : WalkLink::none, true},
                       X, nv, p, G, loss16);
}

// Product 1 runs plain whatever the loss; the resample link kernel leaves R and the partials (with oob the partials alone).
int fos_gradient_batch_resampled(const float* X, int nv, const uint64_t* counts, int oob, fos_problem* p, float* G, double* loss16) {
  const char* fn = "fos_gradient_batch_resampled";
  if (!X || !counts || !p || nv < 1 || nv > fos::BT_NV || ((uintptr_t)counts & 7) != 0 || oob < 0 || oob > 1 || (oob ? !loss16 : !G))
    return fail(FOS_ERR_ARG, std::string(fn) + ": bad argument (null pointer, nv outside 1..16, counts not 8-byte aligned or oob "
                             "outside 0..1)");
  if (int rc = resample_refusal(p, fn, "the resampled data term needs b")) return rc;
  GradientWalk w{fn, "the resampled data term needs b", true, WalkLink::resample, true};
  w.counts = counts; w.oob = oob;
  return gradient_walk(w, X, nv, p, G, loss16);
}

int fos_gather_columns(const int32_t* idx, int32_t n_ws, void* A_ws, int64_t lda_ws, int32_t n_ws_pad, const fos_problem* p) {
  if (!idx || !A_ws || !p) return fail(FOS_ERR_ARG, "fos_gather_columns: null pointer");
  if (n_ws < 1 || n_ws > p->n) return fail(FOS_ERR_ARG, "fos_gather_columns: n_ws outside 1..n");
  if (n_ws_pad < n_ws || n_ws_pad % 8 != 0) return fail(FOS_ERR_ARG, "fos_gather_columns: n_ws_pad is below n_ws or not a multiple of 8");
  if (lda_ws < n_ws_pad || lda_ws % 8 != 0) return fail(FOS_ERR_ARG, "fos_gather_columns: lda_ws is below n_ws_pad or not a multiple of 8");
  if (((uintptr_t)A_ws & 15) != 0) return fail(FOS_ERR_ARG, "fos_gather_columns: A_ws is not 16-byte aligned");
  // whole rows per workgroup, a multiple of the rows in flight; up to four workgroups (32 KiB of LDS each) per CU
  int64_t rows_per_wg = (p->m + 4 * (int64_t)p->ncu - 1) / (4 * (int64_t)p->ncu);
  rows_per_wg = (rows_per_wg + fos::WS_ROWS - 1) / fos::WS_ROWS * fos::WS_ROWS;
  const unsigned grid = (unsigned)((p->m + rows_per_wg - 1) / rows_per_wg);
  if (p->dtype == FOS_BF16)
    hipLaunchKernelGGL(fos::gather_columns_kernel<2>, dim3(grid), dim3(fos::WS_THREADS), 0, p->stream, p->A, p->lda, p->m, (int)p->n, idx,
                       (int)n_ws, (int)n_ws_pad, A_ws, lda_ws, rows_per_wg);
  else
    hipLaunchKernelGGL(fos::gather_columns_kernel<4>, dim3(grid), dim3(fos::WS_THREADS), 0, p->stream, p->A, p->lda, p->m, (int)p->n, idx,
                       (int)n_ws, (int)n_ws_pad, A_ws, lda_ws, rows_per_wg);
  LAUNCH_CHECK();
  return FOS_OK;
}

int fos_kkt_scan(const float* G, int nv, const double* alpha1, double slack, const uint8_t* in_ws, fos_problem* p, float* excess,
                 int32_t* viol_idx, int32_t* viol_count) {
  if (!G || !alpha1 || !in_ws || !p || !excess || !viol_idx || !viol_count || nv < 1 || nv > fos::BT_NV)
    return fail(FOS_ERR_ARG, "fos_kkt_scan: bad argument (null pointer or nv outside 1..16)");
  if (!(std::isfinite(slack) && slack >= 0.0)) return fail(FOS_ERR_ARG, "fos_kkt_scan: slack is not finite and >= 0");
  fos::ClassWeights w;
  if (int rc = class_weights(nv, alpha1, nullptr, "fos_kkt_scan", &w)) return rc;
  if (p->coord_lo || p->coord_hi)
    return fail(FOS_ERR_UNSUPPORTED, "fos_kkt_scan: box bounds (fos_coord_bind) are bound; a coordinate at a bound has another "
                                     "optimality condition");
  if (has_fgroups(p))
    return fail(FOS_ERR_UNSUPPORTED, "fos_kkt_scan: feature groups (fos_feature_groups_bind) are bound; the group norm has another "
                                     "optimality condition");
  if (p->loss == FOS_LOSS_MULTINOMIAL)
    return fail(FOS_ERR_UNSUPPORTED, "fos_kkt_scan: a multinomial problem is not served (squared and logistic loss)");
  hipLaunchKernelGGL(fos::kkt_scan_kernel, dim3(1), dim3(fos::KS_THREADS), 0, p->stream, G, p->n, nv, w, 1.0 + slack, in_ws,
                     p->coord_factor, excess, viol_idx, viol_count);
  LAUNCH_CHECK();
  return FOS_OK;
}

}  // extern "C"

// The row pass of fos_duality_gap on the `rows` rows of p->multi.rbuf16 that product 1 in its plain storing form has just filled
// with Z of the panel starting at row0: one lane per 16-byte quad of a row, grid-stride, at most 2 * ncu workgroups; *nwg_out =
// the rows of `part` written.
static int launch_dual_link(fos_problem* p, int64_t row0, int64_t rows, int nv, const double* scale, double* part, int* nwg_out) {
  const int nwg = (int)std::min<int64_t>((4 * rows + fos::DL_THREADS - 1) / fos::DL_THREADS, 2 * (int64_t)p->ncu);
  const float* w = p->row_weight ? p->row_weight + row0 : nullptr;
  const float c = (float)p->link_param;
#define FOS_DUAL(K, W)                                                                                                      \
  hipLaunchKernelGGL((fos::dual_link_kernel<fos::K, W>), dim3(nwg), dim3(fos::DL_THREADS), 0, p->stream,                   \
                     (const float*)p->multi.rbuf16.get(), rows, p->b + row0, c, nv, w, scale, part)
#define FOS_DUAL_FORM(K) { if (w) FOS_DUAL(K, true); else FOS_DUAL(K, false); }
  switch (p->loss) {
    case FOS_LOSS_SQUARED: FOS_DUAL_FORM(DUAL_SQUARED) break;
    case FOS_LOSS_LOGISTIC: FOS_DUAL_FORM(DUAL_LOGISTIC) break;
    case FOS_LOSS_HUBER: FOS_DUAL_FORM(DUAL_HUBER) break;
    case FOS_LOSS_SQUARED_HINGE: FOS_DUAL_FORM(DUAL_SQUARED_HINGE) break;
    default: return fail(FOS_ERR_STATE, "launch_dual_link: the loss has no conjugate here");
  }
#undef FOS_DUAL_FORM
#undef FOS_DUAL
  LAUNCH_CHECK();
  *nwg_out = nwg;
  return FOS_OK;
}

// The row pass of fos_multinomial_duality_gap, on the logits of the panel likewise: one thread per row, grid-stride, at most ncu
// workgroups.
static int launch_dual_softmax(fos_problem* p, int64_t row0, int64_t rows, int nv, const double* col, double* part, int* nwg_out) {
  const int nwg = (int)std::min<int64_t>((rows + fos::SL_THREADS - 1) / fos::SL_THREADS, p->ncu);
  const float* w = p->row_weight ? p->row_weight + row0 : nullptr;
  if (w)
    hipLaunchKernelGGL(fos::dual_softmax_kernel<true>, dim3(nwg), dim3(fos::SL_THREADS), 0, p->stream,
                       (const float*)p->multi.rbuf16.get(), rows, p->b + row0, p->classes, nv, w, col, part);
  else
    hipLaunchKernelGGL(fos::dual_softmax_kernel<false>, dim3(nwg), dim3(fos::SL_THREADS), 0, p->stream,
                       (const float*)p->multi.rbuf16.get(), rows, p->b + row0, p->classes, nv, w, col, part);
  LAUNCH_CHECK();
  *nwg_out = nwg;
  return FOS_OK;
}

// The row pass of a certificate: its launcher and the rows of the partial buffer it writes per panel at most, in units of ncu.
struct RowPass {
  const char* fn;        // the entry point, for the message
  int (*launch)(fos_problem* p, int64_t row0, int64_t rows, int nv, const double* col, double* part, int* nwg_out);
  int per_cu;
};

// A certificate after its gradient block G (the gradient walk has planned the lockstep and left X packed in cand.xp): the column
// pass - the scale of every fit, then its penalty and the conjugate of the ridge-carrying coordinates -, Z = A_panel X once more
// (plain: no b, no weights, no mask) with the row pass on it, and the finish.
static int certificate_tail(const RowPass& row, const float* X, const float* G, int nv, int classes, int grouped,
                            const fos::ClassWeights& wts, fos_problem* p, double* out64) {
  const int64_t panels = (p->m + p->multi.panel_rows - 1) / p->multi.panel_rows;
  const size_t part_rows = (size_t)panels * 2 * (size_t)p->ncu;
  int rc = p->ws.dual_part.reserve(part_rows * fos::DL_WIDTH);
  if (rc) return rc;
  if ((rc = p->ws.dual_col.reserve(3 * fos::BT_NV))) return rc;
  hipLaunchKernelGGL(fos::dual_scale_kernel, dim3(nv / classes), dim3(fos::DS_THREADS), 0, p->stream, X, G, p->n, classes, grouped, wts,
                     p->coord_factor, p->ws.dual_col.get());
  LAUNCH_CHECK();
  const int64_t esz = p->dtype == FOS_BF16 ? 2 : 4;
  int nparts = 0;
  for (int64_t row0 = 0; row0 < p->m; row0 += p->multi.panel_rows) {
    const int64_t rows = std::min<int64_t>(p->multi.panel_rows, p->m - row0);
    int nwg1 = 0, nwg = 0;
    BatchLaunch L{};
    L.A = reinterpret_cast<const char*>(p->A) + (size_t)row0 * p->lda * esz; L.rows = rows; L.rout = p->multi.rbuf16;
    if ((rc = launch_batch_product(p, L, &nwg1))) return rc;
    if ((size_t)nparts + (size_t)row.per_cu * (size_t)p->ncu > part_rows)
      return fail(FOS_ERR_STATE, std::string(row.fn) + ": the row pass has more panels than its partial buffer holds");
    if ((rc = row.launch(p, row0, rows, nv, p->ws.dual_col, p->ws.dual_part + (size_t)nparts * fos::DL_WIDTH, &nwg))) return rc;
    nparts += nwg;
  }
  hipLaunchKernelGGL(fos::dual_finish_kernel, dim3(1), dim3(fos::DF_THREADS), 0, p->stream, (const double*)p->ws.dual_part.get(), nparts,
                     (const double*)p->ws.dual_col.get(), nv, out64);
  LAUNCH_CHECK();
  return FOS_OK;
}

extern "C" {

int fos_duality_gap(const float* X, int nv, const double* alpha1, const double* alpha2, fos_problem* p, float* G, double* out64) {
  if (!X || !alpha1 || !alpha2 || !p || !G || !out64 || nv < 1 || nv > fos::BT_NV)
    return fail(FOS_ERR_ARG, "fos_duality_gap: bad argument (null pointer or nv outside 1..16)");
  fos::ClassWeights wts;
  int rc = class_weights(nv, alpha1, alpha2, "fos_duality_gap", &wts);
  if (rc) return rc;
  if (p->loss == FOS_LOSS_MULTINOMIAL)
    return fail(FOS_ERR_UNSUPPORTED, "fos_duality_gap: a multinomial problem is not served (squared, logistic, Huber and squared-hinge loss)");
  if ((rc = need_two_products(p, "fos_duality_gap", "the certificate needs b"))) return rc;    // (before the gradient's own: in these words)
  if (p->coord_lo || p->coord_hi)
    return fail(FOS_ERR_UNSUPPORTED, "fos_duality_gap: box bounds (fos_coord_bind) are bound; the penalty of a bounded coordinate has "
                                     "another conjugate");
  if (has_fgroups(p))
    return fail(FOS_ERR_UNSUPPORTED, "fos_duality_gap: feature groups (fos_feature_groups_bind) are bound; the group norm has another "
                                     "conjugate");
  // 1. the gradient block, by the launches of fos_gradient_batch (it plans the lockstep and leaves X packed in cand.xp)
  if ((rc = fos_gradient_batch(X, nv, p, G, nullptr))) return rc;
  // 2. - 4. the column pass (every column a fit of its own, l1), the row pass on Z = A_panel X and the finish
  return certificate_tail({"fos_duality_gap", launch_dual_link, 2}, X, G, nv, 1, 0, wts, p, out64);
}

// The class gradients at the nv columns of X: product 1 runs plain (the logits), the softmax link kernel leaves the residuals in
// place and the loss partials.
int fos_multinomial_gradient_batch(const float* X, int nv, fos_problem* p, float* G, double* loss16) {
  const char* fn = "fos_multinomial_gradient_batch";
  if (!X || !p || !G || nv < 1 || nv > fos::BT_NV)
    return fail(FOS_ERR_ARG, std::string(fn) + ": bad argument (null pointer or nv outside 1..16)");
  if (int rc = need_class_segments(p, nv, fn)) return rc;
  return gradient_walk({fn, "the gradient of the data term needs the labels", true, WalkLink::softmax, false}, X, nv, p, G, loss16);
}

int fos_multinomial_kkt_scan(const float* G, int nv, int grouped, const double* alpha1, double slack, const uint8_t* in_ws,
                             fos_problem* p, float* excess, int32_t* viol_idx, int32_t* viol_count) {
  const char* fn = "fos_multinomial_kkt_scan";
  if (!G || !alpha1 || !in_ws || !p || !excess || !viol_idx || !viol_count || nv < 1 || nv > fos::BT_NV || grouped < 0 || grouped > 1)
    return fail(FOS_ERR_ARG, std::string(fn) + ": bad argument (null pointer, nv outside 1..16 or grouped outside 0..1)");
  if (!(std::isfinite(slack) && slack >= 0.0)) return fail(FOS_ERR_ARG, std::string(fn) + ": slack is not finite and >= 0");
  int rc = need_class_segments(p, nv, fn);
  if (rc) return rc;
  fos::ClassWeights w;
  if ((rc = class_weights(nv / p->classes, alpha1, nullptr, fn, &w))) return rc;
  if (p->coord_lo || p->coord_hi)
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": box bounds (fos_coord_bind) are bound; a coordinate at a bound has another "
                                     "optimality condition");
  hipLaunchKernelGGL(fos::class_kkt_scan_kernel, dim3(1), dim3(fos::KS_THREADS), 0, p->stream, G, p->n, nv, p->classes, grouped, w,
                     1.0 + slack, in_ws, p->coord_factor, excess, viol_idx, viol_count);
  LAUNCH_CHECK();
  return FOS_OK;
}

int fos_multinomial_duality_gap(const float* X, int nv, int grouped, const double* alpha1, const double* alpha2, fos_problem* p,
                                float* G, double* out64) {
  const char* fn = "fos_multinomial_duality_gap";
  if (!X || !alpha1 || !alpha2 || !p || !G || !out64 || nv < 1 || nv > fos::BT_NV || grouped < 0 || grouped > 1)
    return fail(FOS_ERR_ARG, std::string(fn) + ": bad argument (null pointer, nv outside 1..16 or grouped outside 0..1)");
  int rc = need_class_segments(p, nv, fn);
  if (rc) return rc;
  fos::ClassWeights wts;
  if ((rc = class_weights(nv / p->classes, alpha1, alpha2, fn, &wts))) return rc;
  if (p->coord_lo || p->coord_hi)
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": box bounds (fos_coord_bind) are bound; the penalty of a bounded coordinate "
                                     "has another conjugate");
  if (has_fgroups(p))
    return fail(FOS_ERR_UNSUPPORTED, std::string(fn) + ": feature groups (fos_feature_groups_bind) are bound; the group norm has "
                                     "another conjugate");
  // first the class gradients, by the launches of fos_multinomial_gradient_batch (its refusals; it plans the lockstep and leaves X packed)
  if ((rc = fos_multinomial_gradient_batch(X, nv, p, G, nullptr))) return rc;
  return certificate_tail({fn, launch_dual_softmax, 1}, X, G, nv, p->classes, grouped, wts, p, out64);
}

}  // extern "C"
