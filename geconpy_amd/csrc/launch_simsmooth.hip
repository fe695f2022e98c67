// Launcher of the simulation smoother's two kernels (dsge_simsmooth.hpp): the filter means of every path over the stored
// covariance recursion, then the smoother's mean recursion with the draws added back.
#include "dsge_host.hpp"
#include "dsge_simsmooth.hpp"

namespace dsge_host {

int launch_simulation_smoother(const double* T, const ShockCov& q, const ObsModel& o, int batch, int m, int k, int n_paths,
                               const double* U, const double* UT, const double* UR, const int32_t* rank, const double* p_pred,
                               const double* p_filt, const double* xp, const double* eps, long long eps_draw, const double* eta,
                               long long eta_draw, double* a_pred, double* a_filt, double* x_out, double* e_out, int32_t* status,
                               int32_t* snap, hipStream_t st) {
  dsge::SsArgs a{};
  a.T = T; a.Q = q.Q; a.Z = o.Z; a.d = o.d; a.Hdiag = o.Hdiag; a.y = o.y; a.U = U; a.UT = UT; a.UR = UR; a.rank = rank;
  a.p_pred = p_pred; a.p_filt = p_filt; a.xp = xp; a.eps = eps; a.eta = eta; a.eps_draw = eps_draw; a.eta_draw = eta_draw;
  a.a_pred = a_pred; a.a_filt = a_filt; a.x_out = x_out; a.e_out = e_out; a.status = status; a.snap = snap; a.batch = batch; a.m = m;
  a.k = k; a.p = o.p; a.T_len = o.T_len; a.n_paths = n_paths; a.groups = (n_paths + dsge::SS_COLS - 1) / dsge::SS_COLS;
  a.q_mode = q.mode; a.z_batched = o.z_batched; a.d_batched = o.d_batched; a.h_batched = o.h_batched; a.cv = filter_conv(o.jitter);
  a.missing_fill = o.missing_fill;
  const size_t lds_f = dsge::ssf_lds_doubles(m, o.p) * sizeof(double), lds_b = dsge::ssb_lds_doubles(m) * sizeof(double);
  const char* too_large = "simulation smoother: LDS budget exceeded";
  if (lds_f > LDS_LIMIT || lds_b > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, too_large);  // (before the grid's refusal and any launch)
  unsigned grid;
  if (int rc = batch_grid(batch, a.groups, "simulation smoother: batch x path groups exceeds the grid", &grid)) return rc;
  if (int rc = launch_with_lds(dsge::simsmooth_forward_kernel, grid, dsge::SS_THREADS, lds_f, st, a, too_large)) return rc;
  if (dsge::ss_u_global(m)) return launch_with_lds(dsge::simsmooth_backward_kernel<true>, grid, dsge::SS_THREADS, lds_b, st, a, too_large);
  return launch_with_lds(dsge::simsmooth_backward_kernel<false>, grid, dsge::SS_THREADS, lds_b, st, a, too_large);
}

}  // namespace dsge_host
