// Batches of small independent problems in ONE launch: one workgroup per problem, each running the LDS-resident loop of
// resident.hpp on its own A, b, parameters and state.  Nothing crosses workgroups - no grid barrier, no shared word, no
// co-residency assumption - so a problem computes exactly what the one-problem kernel computes on it, and a problem with
// NaN input leaves the others alone.  The SMALL rule of the one-problem path (n <= RS_CHUNK and m <= RS_SMALL_M: rows of
// A in registers) is a template argument here too; the host launches each class over its own range of descriptors.
#pragma once
#include "../../include/fos.h"
#include "resident.hpp"

namespace fos {

// One problem of a FISTA batch, as the device reads it (built by fos_fista_run_batch from fos_batch_item and
// fos_fista_params).  idx: the problem's place in the caller's outputs.
struct ResidentBatchDesc {
  int64_t a_offset, lda, b_offset;   // elements
  int m, n, idx, pad_;
  FistaParams prm;
};

// Outputs of a FISTA batch, problem idx at: x_out + idx*ldx (n doubles), iters_done / stopped / tau_final [idx]; the
// nullable per-iteration records at ls_out / tau_out + idx*iters, hist + idx*iters*4, x_hist + idx*iters*ldx (row stride
// ldx).  scal / x_prev: the state of problem idx (workspace).
struct ResidentBatchOut {
  int64_t ldx;
  double* x_out;
  int* iters_done;
  int* stopped;
  double* tau_final;
  int* ls_out;
  double* tau_out;
  double* hist;
  double* x_hist;
  FistaScalars* scal;
  double* x_prev;
};

// Occupancy (kernel-resource-usage, gfx950): LDS (59 KiB) allows two workgroups per CU; registers decide.  SMALL = false
// takes 123 VGPRs, so two workgroups (4 waves per SIMD) share a CU; SMALL = true keeps its rows of A in registers at 155
// VGPRs, one workgroup per CU (bounding it to 128 spills 89 registers).
template <typename T, bool SMALL>
__global__ __launch_bounds__(RS_THREADS) void fista_resident_batch_kernel(const T* __restrict__ A,
                                                                            const float* __restrict__ B,
                                                                            const ResidentBatchDesc* __restrict__ desc,
                                                                            int iters, int backtracking, double eta,
                                                                            double armijo_c, ResidentBatchOut o) {
  const ResidentBatchDesc d = desc[blockIdx.x];
  const int tid = threadIdx.x;
  const int64_t i = d.idx;
  double* x_cur = o.x_out + i * o.ldx;
  double* x_prev = o.x_prev + i * o.ldx;
  FistaScalars* scal = o.scal + i;
  // the reference's initial state (iterative_solvers.py:160-168): x = 0, t = 1, beta = 0, k = 0 (fista_init_scalars_kernel)
  if (tid < d.n) {
    x_cur[tid] = 0.0;
    x_prev[tid] = 0.0;
  }
  if (tid == 0) {
    FistaScalars z{};
    z.t_prev = 1.0;
    z.ratio = INFINITY;
    *scal = z;
  }
  __syncthreads();                   // the body reads the state back through global memory, workgroup scope
  ResidentOpts opt{backtracking, eta, armijo_c, d.prm.tol_grad,
                   o.ls_out ? o.ls_out + i * iters : nullptr, o.tau_out ? o.tau_out + i * iters : nullptr,
                   o.tau_final + i, o.iters_done + i};
  fista_resident_run<T, SMALL>(A + d.a_offset, d.lda, B + d.b_offset, d.m, d.n, x_cur, x_prev, scal, d.prm, iters,
                               o.x_hist ? o.x_hist + i * iters * o.ldx : nullptr, o.ldx,
                               o.hist ? o.hist + i * iters * 4 : nullptr, opt);
  if (tid == 0) o.stopped[i] = scal->stopped;        // written by this thread at the end of the body
}

// One power iteration (iterative_solvers.py:45-60) per workgroup: problem i = blockIdx.x normalises its own v0 (v_inout +
// i*ldv) and writes L_out[i] and iters_used[i].
template <typename T>
__global__ __launch_bounds__(RS_THREADS) void power_resident_batch_kernel(const T* __restrict__ A,
                                                                            const fos_batch_item* __restrict__ items,
                                                                            float* __restrict__ v_inout, int64_t ldv,
                                                                            int n_iter, double tol,
                                                                            double* __restrict__ L_out,
                                                                            int* __restrict__ iters_used) {
  const int64_t i = blockIdx.x;
  const fos_batch_item it = items[i];
  power_resident_run<T>(A + it.a_offset, it.lda, it.m, it.n, v_inout + i * ldv, n_iter, tol, nullptr, L_out + i,
                        iters_used + i);
}

}  // namespace fos
