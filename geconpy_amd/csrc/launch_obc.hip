// Launcher of the paths under an occasionally binding bound (dsge_obc.hpp), a chain on the caller's stream: the setup kernel of the
// anticipated-shock paths once; its paths kernel on the H unit-shock paths of the constrained column (observed through c: Mz), in
// chunks of draws that keep the parked anticipation terms within 256 MB; the same kernel on the caller's shocks over the first H
// periods; the regime kernel; the paths kernel on e' = e + nu e_s into the caller's outputs; the gap kernel.  The two kernels of
// dsge_anticipated.hpp are launched through launch_anticipated (launch_anticipated.hip), one phase at a time.
#include "dsge_host.hpp"
#include "dsge_obc.hpp"

namespace dsge_host {

int constrained_chunk(int batch, int m, int horizon) {
  const size_t per_draw = (size_t)horizon * horizon * m * sizeof(double), cap = (size_t)256 << 20;
  const size_t fit = cap / per_draw;  // (>= 128: a draw takes at most 2 MB)
  const size_t chunks = ((size_t)batch + fit - 1) / fit;  // ... of equal size
  return chunks <= 1 ? batch : (int)(((size_t)batch + chunks - 1) / chunks);
}

// G, the flag and Mz of every draw (steps 1 and 2 of launch_constrained; launch_obc_sim.hip runs the same chain)
int launch_constrained_mz(const ConstrainedProblem& c, const ConstrainedBuffers& b, hipStream_t st) {
  const AnticipatedProblem& p = c.a;
  const int H = c.horizon, m = p.m, k = p.k;

  // 1. G and the flag of every draw
  if (int rc = launch_anticipated(p, b.B, b.C, b.T, b.R, nullptr, nullptr, nullptr, nullptr, b.status, b.G, 0, b.flag, nullptr, nullptr,
                                  nullptr, nullptr, st, ANT_SETUP))
    return rc;

  // 2. Mz: H unit-shock paths from x0 = 0, observed through c alone (Z = c, d = 0, p = 1)
  const int hk = H * H * k;
  hipLaunchKernelGGL(dsge::obc_unit_kernel, dim3((hk + dsge::OBC_THREADS - 1) / dsge::OBC_THREADS), dim3(dsge::OBC_THREADS), 0, st,
                     b.unit, H, k, c.shock);
  HIP_TRY(hipGetLastError());
  const int chunk = constrained_chunk(p.batch, m, H);
  for (int d0 = 0; d0 < p.batch; d0 += chunk) {
    const size_t o = (size_t)d0;
    AnticipatedProblem u{};
    u.batch = p.batch - d0 < chunk ? p.batch - d0 : chunk;
    u.m = m; u.k = k; u.p = 1; u.n_paths = H; u.n_steps = H; u.n_shock_steps = H; u.mode = DSGE_ANT_PERFECT_FORESIGHT;
    u.z_batched = c.c_batched; u.rank_tol = p.rank_tol;
    if (int rc = launch_anticipated(u, nullptr, nullptr, b.T + o * m * m, b.R + o * m * k, b.unit, nullptr,
                                    b.c_row + (c.c_batched ? o * m : 0), nullptr, b.status ? b.status + o : nullptr, b.G + o * m * m, 0,
                                    b.flag + o, b.mzpark, nullptr, nullptr, b.mzt + o * H * H, st, ANT_PATHS))
      return rc;
  }
  return DSGE_SUCCESS;
}

int launch_constrained(const ConstrainedProblem& c, const ConstrainedBuffers& b, hipStream_t st) {
  const AnticipatedProblem& p = c.a;
  const int H = c.horizon, m = p.m, k = p.k;
  const int nsp = p.n_shock_steps > H ? p.n_shock_steps : H;
  const bool final_paths = b.x_out || b.w_out || b.obs_out || b.gap_out || b.path_status_out;
  const int groups = (p.n_paths + dsge::OBC_WAVES - 1) / dsge::OBC_WAVES;
  unsigned grid;
  if (int rc = batch_grid(p.batch, groups, "constrained paths: batch x path groups exceeds the grid", &grid)) return rc;

  // 1., 2. G, the flag and Mz
  if (int rc = launch_constrained_mz(c, b, st)) return rc;

  // 3. the unconstrained paths, periods < H, into the x buffer
  AnticipatedProblem q = p;
  q.p = 0; q.n_steps = H;
  if (int rc = launch_anticipated(q, nullptr, nullptr, b.T, b.R, b.eps, b.x0, nullptr, nullptr, b.status, b.G, 0, b.flag, b.xbuf, b.xbuf,
                                  nullptr, nullptr, st, ANT_PATHS))
    return rc;

  // 4. the regime iteration
  dsge::ObcArgs r{};
  r.mzt = b.mzt; r.xu = b.xbuf; r.c_row = b.c_row; r.bound = b.bound; r.eps = b.eps; r.status = b.status; r.flag = b.flag;
  r.eps2 = b.eps2; r.qmax = b.qmax; r.pstat = b.pstat; r.nu_out = b.nu_out; r.Mz_out = b.Mz_out; r.iters_out = b.iters_out;
  r.pstat_out = b.path_status_out; r.gap_out = b.gap_out; r.x_out = b.x_out; r.w_out = b.w_out; r.obs_out = b.obs_out;
  r.eps_draw = p.eps_batched ? (long long)p.n_paths * p.n_shock_steps * k : 0;
  r.rank_tol = p.rank_tol;
  r.batch = p.batch; r.m = m; r.k = k; r.p = p.p; r.n_paths = p.n_paths; r.n_steps = p.n_steps; r.n_shock_steps = p.n_shock_steps;
  r.nsp = nsp; r.H = H; r.shock = c.shock; r.max_iter = c.max_iter; r.c_batched = c.c_batched; r.b_batched = c.bound_batched;
  r.groups = groups;
  const size_t lds_regime = dsge::obc_lds_doubles(H) * sizeof(double);
  const char* too_large = "constrained paths: the LDS image exceeds 160 KB";
  if (int rc = H <= 32 ? launch_with_lds(dsge::obc_regime_kernel<32>, grid, dsge::OBC_THREADS, lds_regime, st, r, too_large)
                       : launch_with_lds(dsge::obc_regime_kernel<64>, grid, dsge::OBC_THREADS, lds_regime, st, r, too_large))
    return rc;

  // 5. the final paths on e', into the caller's outputs (x into the x buffer, which the gap kernel reads)
  if (final_paths) {
    AnticipatedProblem f = p;
    f.n_shock_steps = nsp; f.eps_batched = 1;
    if (int rc = launch_anticipated(f, nullptr, nullptr, b.T, b.R, b.eps2, b.x0, b.Z, b.d, b.status, b.G, 0, b.flag,
                                    b.w_out ? b.w_out : b.xbuf, b.xbuf, b.w_out, b.obs_out, st, ANT_PATHS))
      return rc;
    r.x = b.xbuf;
  }

  // 6. the gap, the bit beyond the horizon, NaN over failed paths, the draw's word
  hipLaunchKernelGGL(dsge::obc_gap_kernel, dim3(grid), dim3(dsge::OBC_THREADS), 0, st, r);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

}  // namespace dsge_host
