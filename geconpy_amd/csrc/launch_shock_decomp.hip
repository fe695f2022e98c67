// Launcher of the historical shock decomposition (dsge_shock_decomp.hpp): one workgroup per draw and pack of paths.
#include "dsge_host.hpp"
#include "dsge_shock_decomp.hpp"

namespace dsge_host {

long long* g_shock_decomp_dbg = nullptr;  // debug: device int64[8], phase cycles of workgroup 0 (dsge_debug_shock_decomp_phases)

size_t shock_decomp_lds_bytes(int m, int k, int p, int n_groups) {
  return dsge::sd_lds_doubles(m, k, p, dsge::SD_COLS / (n_groups + 1)) * sizeof(double);
}

int launch_shock_decomp(const double* T, const double* R, const double* eps, const double* x, const int32_t* grp, int n_groups,
                        const int32_t* var, int n_out, const double* Z, int z_batched, const int32_t* status, int batch, int m, int k,
                        int p, int n_paths, int T_len, int remainder, double* contrib_out, double* obs_out, hipStream_t st) {
  if (!contrib_out) n_out = 0;
  dsge::ShockDecompArgs a{};
  a.T = T; a.R = R; a.eps = eps; a.x = x; a.Z = Z; a.status = status; a.contrib = contrib_out; a.obs = obs_out; a.batch = batch;
  a.m = m; a.k = k; a.p = p; a.n_paths = n_paths; a.T_len = T_len; a.n_out = n_out; a.g = n_groups; a.remainder = remainder ? 1 : 0;
  a.z_batched = z_batched; a.dbg = g_shock_decomp_dbg;
  a.pack = dsge::SD_COLS / (n_groups + 1);
  a.units = (n_paths + a.pack - 1) / a.pack;
  for (int j = 0; j < k; ++j) a.grp[j] = (unsigned char)(grp ? grp[j] : j);
  for (int i = 0; i < n_out; ++i) a.var[i] = (unsigned char)(var ? var[i] : i);
  const char* too_large = "shock decomposition: [T | R] does not fit the LDS";
  const size_t lds = shock_decomp_lds_bytes(m, k, obs_out ? p : 0, n_groups);
  if (lds > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, too_large);  // (the LDS refusal comes before the grid's)
  unsigned grid;
  if (int rc = batch_grid(batch, a.units, "shock decomposition: batch x path packs exceeds the grid", &grid)) return rc;
  return launch_with_lds(dsge::shock_decomp_kernel, grid, dsge::SD_THREADS, lds, st, a, too_large);
}

}  // namespace dsge_host
