// Launcher of the spectral moments (dsge_spectral.hpp): the solve kernel, one wavefront per draw and frequency group, then the
// reduction, one workgroup per draw, both on the caller's stream.
#include "dsge_host.hpp"
#include "dsge_spectral.hpp"

namespace dsge_host {

size_t spectral_lds_bytes(int m, int k, int p, int has_z) { return dsge::sp_solve_lds_doubles(m, k, p, has_z) * sizeof(double); }

int launch_spectral(const SpectralProblem& s, const double* T, const double* R, const ShockCov& q, const double* Z,
                    const double* Hdiag, const double* gain, int32_t* status, int32_t* flag, double* F, double* acov_out,
                    double* spectrum_out, hipStream_t st) {
  dsge::SpectralArgs a{};
  a.T = T; a.R = R; a.Q = q.Q; a.Z = Z; a.Hdiag = Hdiag; a.gain = gain;
  a.q_mode = q.mode; a.z_batched = s.z_batched; a.h_batched = s.h_batched;
  a.batch = s.batch; a.m = s.m; a.k = s.k; a.p = s.p; a.dim = Z ? s.p : s.m; a.n_grid = s.n_grid; a.nf = s.n_grid / 2 + 1;
  a.n_lags = s.n_lags; a.correlation = s.correlation; a.solve_all = spectrum_out != nullptr; a.rank_tol = s.rank_tol;
  a.status_in = status; a.status = status; a.flag = flag; a.F = reinterpret_cast<double2*>(F); a.acov = acov_out;
  a.spec = reinterpret_cast<double2*>(spectrum_out);
  // enough wavefronts for some twenty rounds over the chip (about 1 500 resident at the timed shape), so that the last round
  // costs little; the result does not depend on the grouping
  int groups = (32768 + s.batch - 1) / s.batch;
  a.groups = groups < 1 ? 1 : (groups > a.nf ? a.nf : groups);
  const size_t lds_solve = spectral_lds_bytes(s.m, s.k, s.p, Z != nullptr);
  const size_t lds_reduce = dsge::sp_reduce_lds_doubles(s.n_grid, a.dim) * sizeof(double);
  const char* too_large = "spectral moments: the LDS image exceeds 160 KB";
  if (lds_solve > LDS_LIMIT || lds_reduce > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, too_large);  // (before anything is enqueued)
  unsigned grid;
  int rc;
  if ((rc = batch_grid(s.batch, a.groups, "spectral moments: batch x frequency groups exceeds the grid", &grid))) return rc;
  HIP_TRY(hipMemsetAsync(flag, 0, (size_t)s.batch * sizeof(int32_t), st));
  // NC: the register row of the solve kernel, the multiple of 16 that holds m + k complex entries
#define SPECTRAL_SOLVE(NC) rc = launch_with_lds(dsge::spectral_solve_kernel<NC>, grid, 64, lds_solve, st, a, too_large)
  switch ((s.m + s.k + 15) / 16) {
    case 1: SPECTRAL_SOLVE(16); break;
    case 2: SPECTRAL_SOLVE(32); break;
    case 3: SPECTRAL_SOLVE(48); break;
    case 4: SPECTRAL_SOLVE(64); break;
    case 5: SPECTRAL_SOLVE(80); break;
    case 6: SPECTRAL_SOLVE(96); break;
    default: return fail(DSGE_ERR_TOO_LARGE, "spectral moments: m + k exceeds 96");
  }
#undef SPECTRAL_SOLVE
  if (rc) return rc;
  return launch_with_lds(dsge::spectral_reduce_kernel, s.batch, dsge::SP_REDUCE_THREADS, lds_reduce, st, a, too_large);
}

}  // namespace dsge_host
