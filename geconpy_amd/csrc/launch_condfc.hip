// Launcher of the conditional forecast (dsge_condfc.hpp): the setup kernel, one workgroup per draw, then the paths kernel, one
// workgroup per draw and group of 16 paths, both on the caller's stream.
#include "dsge_host.hpp"
#include "dsge_condfc.hpp"

namespace dsge_host {

long long* g_condfc_dbg = nullptr;  // debug: device int64[8], phase cycles of workgroup 0 of both kernels (dsge_debug_condfc_phases)

size_t condfc_lds_bytes(int m, int k, int p, int n_cond, int lags, int n_free) {
  const size_t setup = n_cond > 0 ? dsge::cf_setup_lds_doubles(m, k, n_cond) : 0;
  const size_t paths = dsge::cf_paths_lds_doubles(m, k, p, n_cond, n_cond > 0 ? lags : 0, n_free);
  return (setup > paths ? setup : paths) * sizeof(double);
}

int launch_condfc(const CondFcProblem& c, const double* T, const double* R, const ShockCov& q, const double* Z, int z_batched,
                  const double* d, int d_batched, const double* x0, const double* eps, const double* cond_val, int32_t* status,
                  double* chol, double* psi, double* psiq, int32_t* flag, double* x_out, double* eps_out, double* obs_out,
                  hipStream_t st) {
  dsge::CondFcArgs a{};
  a.T = T; a.R = R; a.Q = q.Q; a.q_mode = q.mode; a.Z = Z; a.z_batched = z_batched; a.d = d; a.d_batched = d_batched;
  a.x0 = x0; a.x0_path = c.x0_paths ? c.m : 0; a.x0_draw = c.x0_batched ? (long long)(c.x0_paths ? c.n_paths : 1) * c.m : 0;
  a.eps = eps; a.eps_draw = c.eps_batched ? (long long)c.n_paths * c.n_shock_steps * c.k : 0;
  a.cond_val = cond_val; a.cv_path = c.cv_paths ? c.n_cond : 0;
  a.cv_draw = c.cv_batched ? (long long)(c.cv_paths ? c.n_paths : 1) * c.n_cond : 0;
  a.status = status; a.x_out = x_out; a.eps_out = eps_out; a.obs_out = obs_out; a.chol = chol; a.psi = psi; a.psiq = psiq;
  a.flag = flag; a.dbg = g_condfc_dbg; a.rank_tol = c.rank_tol;
  a.batch = c.batch; a.m = c.m; a.k = c.k; a.p = c.p; a.n_paths = c.n_paths; a.n_steps = c.n_steps;
  a.n_shock_steps = c.n_shock_steps; a.n_cond = c.n_cond; a.t_max = c.t_max; a.n_free = c.n_free;
  a.groups = (c.n_paths + dsge::CF_COLS - 1) / dsge::CF_COLS;
  for (int i = 0; i < c.n_cond; ++i) {
    a.cond_t[i] = c.cond_t[i];
    a.cond_j[i] = (unsigned char)c.cond_j[i];
  }
  int nf = 0;
  for (int j = 0; j < c.k; ++j) {
    const bool free_j = !c.free_shock || c.free_shock[j] != 0;
    a.free_pos[j] = free_j ? (signed char)nf : (signed char)-1;
    if (free_j) a.free_idx[nf++] = (unsigned char)j;
  }
  const size_t lds_setup = c.n_cond > 0 ? dsge::cf_setup_lds_doubles(c.m, c.k, c.n_cond) * sizeof(double) : 0;
  const size_t lds_paths = dsge::cf_paths_lds_doubles(c.m, c.k, c.p, c.n_cond, c.n_cond > 0 ? c.t_max + 1 : 0, c.n_free) * sizeof(double);
  const char* too_large = "conditional forecast: the LDS image exceeds 160 KB";
  if (lds_setup > LDS_LIMIT || lds_paths > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, too_large);  // (before the grid's refusal and any launch)
  unsigned grid;
  if (int rc = batch_grid(c.batch, a.groups, "conditional forecast: batch x path groups exceeds the grid", &grid)) return rc;
  if (c.n_cond > 0)
    if (int rc = launch_with_lds(dsge::condfc_setup_kernel, c.batch, dsge::CF_THREADS, lds_setup, st, a, too_large)) return rc;
  return launch_with_lds(dsge::condfc_paths_kernel, grid, dsge::CF_THREADS, lds_paths, st, a, too_large);
}

}  // namespace dsge_host
