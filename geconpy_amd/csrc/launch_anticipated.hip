// Launcher of the anticipated-shock paths (dsge_anticipated.hpp): the setup kernel, one workgroup per draw, then (when a path output
// is wanted) the paths kernel, one workgroup per draw and group of 16 paths, both on the caller's stream.
#include "dsge_host.hpp"
#include "dsge_anticipated.hpp"

namespace dsge_host {

size_t anticipated_lds_bytes(int m, int k, int p) {
  const size_t setup = dsge::an_setup_lds_doubles(m), paths = dsge::an_paths_lds_doubles(m, k, p, 1);
  return (setup > paths ? setup : paths) * sizeof(double);
}

int launch_anticipated(const AnticipatedProblem& c, const double* B, const double* C, const double* T, const double* R,
                       const double* eps, const double* x0, const double* Z, const double* d, int32_t* status, double* G,
                       int g_is_out, int32_t* flag, double* park, double* x_out, double* w_out, double* obs_out, hipStream_t st,
                       int phases) {
  dsge::AntArgs a{};
  a.B = B; a.C = C; a.T = T; a.R = R; a.eps = eps; a.x0 = x0; a.Z = Z; a.d = d; a.status = status; a.G = G; a.g_is_out = g_is_out;
  a.flag = flag; a.park = park; a.x_out = x_out; a.w_out = w_out; a.obs_out = obs_out; a.rank_tol = c.rank_tol;
  const int rows = c.n_shock_steps * (c.mode == DSGE_ANT_NEWS ? c.n_lead + 1 : 1);
  a.eps_draw = c.eps_batched ? (long long)c.n_paths * rows * c.k : 0;
  a.x0_path = c.x0_paths ? c.m : 0;
  a.x0_draw = c.x0_batched ? (long long)(c.x0_paths ? c.n_paths : 1) * c.m : 0;
  a.batch = c.batch; a.m = c.m; a.k = c.k; a.p = c.p; a.n_paths = c.n_paths; a.n_steps = c.n_steps;
  a.n_shock_steps = c.n_shock_steps; a.news = c.mode == DSGE_ANT_NEWS; a.n_lead = a.news ? c.n_lead : 0;
  a.z_batched = c.z_batched; a.d_batched = c.d_batched;
  a.groups = (c.n_paths + dsge::AN_COLS - 1) / dsge::AN_COLS;
  const size_t lds_setup = dsge::an_setup_lds_doubles(c.m) * sizeof(double);
  const size_t lds_paths = dsge::an_paths_lds_doubles(c.m, c.k, c.p, 1) * sizeof(double);
  const size_t lds_wide = dsge::an_paths_lds_doubles(c.m, c.k, c.p, dsge::AN_PB) * sizeof(double);
  const char* too_large = "anticipated paths: the LDS image exceeds 160 KB";
  if (lds_setup > LDS_LIMIT || lds_paths > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, too_large);  // (before any launch)
  unsigned grid;
  if (int rc = batch_grid(c.batch, a.groups, "anticipated paths: batch x path groups exceeds the grid", &grid)) return rc;
  if (phases & ANT_SETUP)
    if (int rc = launch_with_lds(dsge::ant_setup_kernel, c.batch, dsge::AN_THREADS, lds_setup, st, a, too_large)) return rc;
  if (!park || !(phases & ANT_PATHS)) return DSGE_SUCCESS;  // G alone
  // News with a lead on a grid of at most WIDE_GRID workgroups (two per CU of a 256-CU device: the steps' latency is not hidden by
  // other workgroups) runs AN_PB periods per Horner step, if its wider images fit; the bits are those of one period per step
  constexpr unsigned WIDE_GRID = 512;
  if (a.news && a.n_lead > 0 && c.n_shock_steps > 1 && grid <= WIDE_GRID && lds_wide <= LDS_LIMIT)
    return launch_with_lds(dsge::ant_paths_kernel<dsge::AN_PB>, grid, dsge::AN_THREADS, lds_wide, st, a, too_large);
  return launch_with_lds(dsge::ant_paths_kernel<1>, grid, dsge::AN_THREADS, lds_paths, st, a, too_large);
}

}  // namespace dsge_host
