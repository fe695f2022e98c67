// Host only: the ONE place where each filter kernel's positional argument list is written.  A launch site fills a FilterArgs and
// names the instance; the function template of the kernel's family sets the LDS size, expands the struct, launches and checks.
// Every kernel header included here holds templates only, so a translation unit instantiates exactly the kernels it launches.
#pragma once
#include "dsge_host.hpp"
#include "dsge_kalman2.hpp"
#include "dsge_kalman_grad.hpp"
#include "dsge_kalman_mf.hpp"
#include "dsge_kalman_nt.hpp"
#include "dsge_kalman_nt2.hpp"
#include "dsge_kalman_tiny.hpp"
#include "dsge_kernels.hpp"

namespace dsge_host {

// What the filter kernels share.  A member left at its default is "not used" by that launch.
struct FilterArgs {
  const double* T = nullptr;
  const double* RQR = nullptr;
  const double* P0 = nullptr;  // null: the fast kernels compute the stationary covariance themselves
  ObsModel o{};
  int batch = 0, m = 0;
  dsge::FilterConv cv{};
  double steady_tol = 0.0;
  double* logp = nullptr;
  int32_t* status = nullptr;
  int s_cap = 0;                  // capacity of the state block (sel, nt, nt2)
  int rerun = 0;                  // 1: second pass, only the draws flagged DSGE_ST_INTERNAL_RERUN
  const int32_t* order = nullptr;  // dispatch order
  const double* Rsel = nullptr;   // selection matrix: the kernel forms sym(R Q R') of its retained block itself (nt, nt2, mf)
  ShockCov q{};
  int k_shocks = 0;
  const unsigned long long* colmask = nullptr;
  double* tail_rec = nullptr;     // hand-off to the tail kernels (sel, nt)
  int32_t* tail_flag = nullptr;
  const int32_t* tail_from = nullptr;
  double* rec_store = nullptr;    // record of the gradient's forward sweep (nt, mf); what kalman_grad_kernel reads
  long long* dbg = nullptr;       // phase stamps or timeline
  int32_t* steady_at = nullptr;   // first steady step per draw
};
// the reverse sweep's outputs
struct GradBars {
  double *Tbar, *Gbar, *dbar, *hbar;
};

template <int U, int PM>
int launch_tiny(unsigned grid, hipStream_t st, const FilterArgs& a) {
  const ObsModel& o = a.o;
  hipLaunchKernelGGL((dsge::kalman_tiny_kernel<U, PM>), dim3(grid), dim3(64), 0, st, a.T, a.RQR, o.Z, o.z_batched, o.d, o.d_batched,
                     o.Hdiag, o.h_batched, o.y, a.batch, a.m, o.p, o.T_len, a.cv, o.missing_fill, a.steady_tol, a.logp, a.status,
                     a.steady_at);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

template <int BS, bool SEL, bool MF = false, bool TAIL = false>
int launch_sel(unsigned grid, hipStream_t st, size_t lds, const FilterArgs& a) {
  const ObsModel& o = a.o;
  if (int rc = set_lds(dsge::kalman_sel_kernel<BS, SEL, MF, TAIL>, lds)) return rc;
  hipLaunchKernelGGL((dsge::kalman_sel_kernel<BS, SEL, MF, TAIL>), dim3(grid), dim3(64), lds, st, a.T, a.RQR, a.P0, o.Z, o.z_batched,
                     o.d, o.d_batched, o.Hdiag, o.h_batched, o.y, a.batch, a.m, o.p, o.T_len, a.s_cap, a.cv, o.missing_fill,
                     a.steady_tol, a.logp, a.status, a.dbg, a.rerun, a.steady_at, a.tail_rec, a.tail_flag, a.tail_from, a.order);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

template <int BS, bool DBG, int SK, bool TAIL = false, bool REC = false>
int launch_nt(unsigned grid, hipStream_t st, size_t lds, const FilterArgs& a) {
  const ObsModel& o = a.o;
  if (int rc = set_lds(dsge::kalman_nt_kernel<BS, DBG, SK, TAIL, REC>, lds)) return rc;
  hipLaunchKernelGGL((dsge::kalman_nt_kernel<BS, DBG, SK, TAIL, REC>), dim3(grid), dim3(64), lds, st, a.T, a.RQR, a.P0, o.Z,
                     o.z_batched, o.d, o.d_batched, o.Hdiag, o.h_batched, o.y, a.batch, a.m, o.p, o.T_len, a.s_cap, a.cv,
                     o.missing_fill, a.steady_tol, a.logp, a.status, a.dbg, a.rerun, a.steady_at, a.order, a.Rsel, a.q.Q,
                     a.q.batched(), a.k_shocks, a.colmask, a.tail_rec, a.tail_flag, a.tail_from, a.rec_store);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

template <int BS, int SK, bool DBG = false>
int launch_nt2(unsigned grid, hipStream_t st, size_t lds, const FilterArgs& a) {
  const ObsModel& o = a.o;
  if (int rc = set_lds(dsge::kalman_nt2_kernel<BS, SK, DBG>, lds)) return rc;
  hipLaunchKernelGGL((dsge::kalman_nt2_kernel<BS, SK, DBG>), dim3(grid), dim3(128), lds, st, a.T, a.RQR, a.P0, o.Z, o.z_batched, o.d,
                     o.d_batched, o.Hdiag, o.h_batched, o.y, a.batch, a.m, o.p, o.T_len, a.s_cap, a.cv, o.missing_fill, a.steady_tol,
                     a.logp, a.status, a.rerun, a.steady_at, a.order, a.Rsel, a.q.Q, a.q.batched(), a.k_shocks, a.colmask, a.dbg);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

template <int KT, int TM, bool DBG, bool REC = false, int RBS = (4 * TM + 7) / 8>
int launch_mf(unsigned grid, hipStream_t st, size_t lds, const FilterArgs& a) {
  const ObsModel& o = a.o;
  if (int rc = set_lds(dsge::kalman_mf_kernel<KT, TM, DBG, REC, RBS>, lds)) return rc;
  hipLaunchKernelGGL((dsge::kalman_mf_kernel<KT, TM, DBG, REC, RBS>), dim3(grid), dim3(64), lds, st, a.T, a.RQR, a.P0, o.Z,
                     o.z_batched, o.d, o.d_batched, o.Hdiag, o.h_batched, o.y, a.batch, a.m, o.p, o.T_len, a.cv, o.missing_fill,
                     a.steady_tol, a.logp, a.status, a.dbg, a.rerun, a.steady_at, a.order, a.Rsel, a.q.Q, a.q.batched(), a.k_shocks,
                     a.colmask, a.rec_store);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

// the general kernel (dsge_kernels.hpp): every draw with its full-size P0
template <int BS>
int launch_general(unsigned grid, hipStream_t st, size_t lds, const FilterArgs& a) {
  const ObsModel& o = a.o;
  if (int rc = set_lds(dsge::kalman_kernel<BS>, lds)) return rc;
  hipLaunchKernelGGL(dsge::kalman_kernel<BS>, dim3(grid), dim3(64), lds, st, a.T, a.RQR, a.P0, o.Z, o.z_batched, o.d, o.d_batched,
                     o.Hdiag, o.h_batched, o.y, a.batch, a.m, o.p, o.T_len, a.cv, o.missing_fill, a.logp, a.status, a.rerun);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

template <int BS, bool SPLIT>
int launch_grad(unsigned grid, hipStream_t st, size_t lds, const FilterArgs& a, const GradBars& g, int tail_valid) {
  const ObsModel& o = a.o;
  if (int rc = set_lds(dsge::kalman_grad_kernel<BS, SPLIT>, lds)) return rc;
  hipLaunchKernelGGL((dsge::kalman_grad_kernel<BS, SPLIT>), dim3(grid), dim3(64), lds, st, a.T, a.RQR, o.Z, o.z_batched, o.d,
                     o.d_batched, o.Hdiag, o.h_batched, o.y, a.batch, a.m, o.p, o.T_len, a.cv, o.missing_fill, a.steady_tol,
                     a.rec_store, a.logp, a.status, g.Tbar, g.Gbar, g.dbar, g.hbar, a.dbg, a.order, a.rerun, tail_valid);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

}  // namespace dsge_host
