// Launchers of the post-solve dynamics kernels (dsge_dynamics.hpp): propagation (simulate, impulse responses, FEVD) and the
// forecast moment recursion.
#include "dsge_host.hpp"
#include "dsge_dynamics.hpp"

namespace dsge_host {

int launch_propagate(const double* T, const double* R, const double* shocks, long long sh_draw, long long sh_path, long long sh_step,
                     long long sh_comp, int identity, const double* x0, long long x0_draw, const double* weights, long long w_draw,
                     const int32_t* status, int batch, int m, int k, int n_paths, int n_steps, int n_shock_steps, double* x_out,
                     double* fevd_out, hipStream_t st) {
  dsge::DynArgs a{};
  a.T = T; a.R = R; a.shocks = shocks; a.sh_draw = sh_draw; a.sh_path = sh_path; a.sh_step = sh_step; a.sh_comp = sh_comp;
  a.identity = identity; a.x0 = x0; a.x0_draw = x0_draw; a.weights = weights; a.w_draw = w_draw; a.status = status; a.x_out = x_out;
  a.fevd = fevd_out; a.batch = batch; a.m = m; a.k = k; a.n_paths = n_paths; a.n_steps = n_steps; a.n_shock_steps = n_shock_steps;
  a.groups = (n_paths + dsge::DY_COLS - 1) / dsge::DY_COLS;
  if (fevd_out && a.groups != 1) return fail(DSGE_ERR_INVALID, "propagate: on-chip FEVD takes one column group");
  const char* too_large = "dynamics: [T | R] does not fit the LDS (m = 96 takes k <= 32)";
  const size_t lds = dsge::dy_lds_doubles(m, k) * sizeof(double);
  if (lds > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, too_large);  // (the LDS refusal comes before the grid's)
  unsigned grid;
  if (int rc = batch_grid(batch, a.groups, "dynamics: batch x path groups exceeds the grid", &grid)) return rc;
  return launch_with_lds(dsge::dynamics_propagate_kernel, grid, dsge::DY_THREADS, lds, st, a, too_large);
}

int launch_fevd(const double* irf, const double* weights, long long w_draw, const int32_t* status, int batch, int m, int c,
                int n_steps, double* fevd_out, hipStream_t st) {
  dsge::FevdArgs a{};
  a.irf = irf; a.weights = weights; a.w_draw = w_draw; a.status = status; a.fevd = fevd_out; a.batch = batch; a.m = m; a.c = c;
  a.n_steps = n_steps;
  return launch_with_lds(dsge::dynamics_fevd_kernel, batch, dsge::DY_THREADS, dsge::dy_fevd_lds_doubles(m, c) * sizeof(double), st, a,
                         "dynamics: the FEVD sums of this many impulses do not fit the LDS");
}

int launch_forecast(const double* T, const double* R, const ShockCov& q, const ObsModel& o, const double* a0, const double* P0,
                    const int32_t* status, int batch, int m, int k, int n_steps, double* a_out, double* p_out, int full_cov,
                    double* y_out, double* f_out, hipStream_t st) {
  dsge::FcArgs a{};
  a.T = T; a.R = R; a.Q = q.Q; a.Z = o.Z; a.d = o.d; a.Hdiag = o.Hdiag; a.a0 = a0; a.P0 = P0; a.status = status; a.a_out = a_out;
  a.p_out = p_out; a.y_out = y_out; a.f_out = f_out; a.batch = batch; a.m = m; a.k = k; a.p = o.p; a.n_steps = n_steps;
  a.q_mode = q.mode; a.z_batched = o.z_batched; a.d_batched = o.d_batched; a.h_batched = o.h_batched; a.full_cov = full_cov;
  return launch_with_lds(dsge::dynamics_forecast_kernel, batch, dsge::FC_THREADS, dsge::fc_lds_doubles(m, o.p) * sizeof(double), st, a,
                         "forecast: LDS budget exceeded");
}

}  // namespace dsge_host
