// Launchers of the second-order dynamics kernels (dsge_pruned.hpp): the panel of the second-order blocks per draw, then the pruned
// recursion for groups of 16 paths (simulate) or for 8 pairs of baseline and shocked paths per impulse (generalised responses).
#include "dsge_host.hpp"
#include "dsge_pruned.hpp"

namespace dsge_host {

long long* g_pruned_dbg = nullptr;  // debug: device int64[8], phase cycles of workgroup 0 (dsge_debug_pruned_phases)

size_t pruned_panel_doubles(int n, int s, int k) { return dsge::pr_panel_doubles(n, s, k); }

int launch_pruned(const PrunedProblem& p, int batch, const double* eps, const double* xf0, const double* xs0, const double* imp,
                  const int32_t* status, double* panel, double* x_out, double* xf_out, double* xs_out, double* girf_out,
                  hipStream_t st) {
  const int n = p.n, s = p.s, k = p.k;
  const size_t lds = dsge::pr_lds_doubles(n, s, k) * sizeof(double);
  const char* too_large = "pruned dynamics: LDS budget exceeded";
  if (lds > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, too_large);  // (before the grid's refusal and the pack kernel)
  const int units = girf_out ? p.c : (p.n_paths + dsge::PR_COLS - 1) / dsge::PR_COLS;
  unsigned grid;
  if (int rc = batch_grid(batch, units, "pruned dynamics: batch x path groups exceeds the grid", &grid)) return rc;
  dsge::PrunedPackArgs pk{};
  pk.gyy = p.gyy; pk.gyu = p.gyu; pk.guu = p.guu; pk.gss = p.gss; pk.status = status; pk.panel = panel; pk.batch = batch; pk.n = n;
  pk.s = s; pk.k = k;
  hipLaunchKernelGGL(dsge::pruned_pack_kernel, dim3(batch), dim3(dsge::PR_THREADS), 0, st, pk);
  HIP_TRY(hipGetLastError());
  dsge::PrunedArgs a{};
  a.T = p.T; a.R = p.R; a.panel = panel; a.eps = eps; a.eps_draw = p.eps_draw; a.xf0 = xf0; a.xs0 = xs0; a.x0_draw = p.x0_draw; a.imp = imp;
  a.imp_draw = p.imp_draw; a.status = status; a.x_out = x_out; a.xf_out = xf_out; a.xs_out = xs_out; a.girf_out = girf_out; a.batch = batch;
  a.n = n; a.s = s; a.k = k; a.n_paths = p.n_paths; a.n_steps = p.n_steps; a.n_shock_steps = p.n_shock_steps; a.units = units;
  a.girf = girf_out ? 1 : 0; a.dbg = g_pruned_dbg;
  for (int i = 0; i < s; ++i) a.S[i] = (unsigned char)p.S[i];
  return launch_with_lds(dsge::pruned_propagate_kernel, grid, dsge::PR_THREADS, lds, st, a, too_large);
}

}  // namespace dsge_host
