// Launcher of the stochastic simulation at an occasionally binding bound (dsge_obc_sim.hpp), a chain on the caller's stream: G, the
// flag and Mz of every draw by the first two steps of launch_constrained (launch_obc.hip) as they are; the tables Cq and W per draw;
// the simulation kernel, the time loop inside it; the draw's status bit.
#include "dsge_host.hpp"
#include "dsge_obc_sim.hpp"

namespace dsge_host {

size_t constrained_sim_lds_bytes(int m, int k, int horizon) {
  return dsge::obc_sim_lds_doubles(horizon, m, k, dsge::obc_sim_r_in_lds(horizon, m, k, LDS_LIMIT)) * sizeof(double);
}

int launch_constrained_sim(const ConstrainedProblem& c, const ConstrainedSimBuffers& b, hipStream_t st) {
  const AnticipatedProblem& p = c.a;
  const int H = c.horizon, m = p.m, k = p.k;
  const int groups = (p.n_paths + dsge::OBC_WAVES - 1) / dsge::OBC_WAVES;
  unsigned grid;
  if (int rc = batch_grid(p.batch, groups, "constrained simulation: batch x path groups exceeds the grid", &grid)) return rc;

  // 1. G, the flag and Mz
  if (int rc = launch_constrained_mz(c, b.mz, st)) return rc;

  // 2. Cq and W
  dsge::ObcSimArgs a{};
  a.T = b.mz.T; a.R = b.mz.R; a.G = b.mz.G; a.mzt = b.mz.mzt; a.c_row = b.mz.c_row; a.bound = b.mz.bound; a.eps = b.mz.eps; a.x0 = b.mz.x0;
  a.Z = b.mz.Z; a.d = b.mz.d; a.status = b.mz.status; a.flag = b.mz.flag; a.cq = b.cq; a.wt = b.wt; a.pstat = b.pstat;
  a.x_out = b.x_out; a.obs_out = b.obs_out; a.gap_out = b.gap_out; a.shadow_out = b.shadow_out; a.plan_out = b.plan_out;
  a.duration_out = b.duration_out; a.iters_out = b.iters_out; a.Mz_out = b.Mz_out; a.pstat_out = b.path_status_out;
  a.fail_out = b.fail_step_out;
  a.eps_draw = p.eps_batched ? (long long)p.n_paths * p.n_shock_steps * k : 0;
  a.rank_tol = p.rank_tol;
  a.batch = p.batch; a.m = m; a.k = k; a.p = p.p; a.n_paths = p.n_paths; a.n_steps = p.n_steps; a.n_shock_steps = p.n_shock_steps;
  a.H = H; a.shock = c.shock; a.max_iter = c.max_iter; a.c_batched = c.c_batched; a.b_batched = c.bound_batched;
  a.x0_batched = p.x0_batched; a.x0_paths = p.x0_paths; a.z_batched = p.z_batched; a.d_batched = p.d_batched; a.groups = groups;
  a.r_lds = dsge::obc_sim_r_in_lds(H, m, k, LDS_LIMIT);
  const char* too_large = "constrained simulation: the LDS image exceeds 160 KB";
  if (int rc = launch_with_lds(dsge::obc_sim_setup_kernel, (unsigned)p.batch, dsge::OBC_SIM_SETUP_THREADS,
                               dsge::obc_sim_setup_lds_doubles(m) * sizeof(double), st, a, too_large))
    return rc;

  // 3. the simulation: R in the LDS where it fits beside the tables (n = H = 64: up to k = 47), else read from global memory
  const size_t lds = constrained_sim_lds_bytes(m, k, H);
  if (int rc = H <= 32 ? launch_with_lds(dsge::obc_sim_kernel<32>, grid, dsge::OBC_THREADS, lds, st, a, too_large)
                       : launch_with_lds(dsge::obc_sim_kernel<64>, grid, dsge::OBC_THREADS, lds, st, a, too_large))
    return rc;

  // 4. the draw's word
  if (b.mz.status) {
    hipLaunchKernelGGL(dsge::obc_sim_status_kernel, dim3((p.batch + dsge::OBC_THREADS - 1) / dsge::OBC_THREADS), dim3(dsge::OBC_THREADS), 0,
                       st, b.mz.status, b.pstat, p.batch, p.n_paths);
    HIP_TRY(hipGetLastError());
  }
  return DSGE_SUCCESS;
}

}  // namespace dsge_host
