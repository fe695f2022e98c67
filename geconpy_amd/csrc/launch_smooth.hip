// Launchers of the fixed-interval smoother (dsge_kalman_smooth.hpp): basis of range(P_pred) per draw, then the backward pass; and of
// the same across dated structural breaks: a basis per (draw, segment), the backward pass with the segment switch.
#include "dsge_host.hpp"
#include "dsge_kalman_smooth.hpp"

namespace dsge_host {

size_t smoother_image_doubles(int m) { return dsge::ks_mat(m); }

// the basis alone (the simulation smoother runs its own backward pass on it)
int launch_smoother_basis(const double* T, const double* R, const ShockCov& q, int batch, int m, int k, double rank_tol, double* U,
                          double* UT, double* UR, int32_t* rank, int32_t* status, hipStream_t st) {
  dsge::KsArgs a{};
  a.T = T; a.R = R; a.Q = q.Q; a.U = U; a.UT = UT; a.UR = UR; a.rank = rank; a.status = status; a.batch = batch; a.m = m; a.k = k;
  a.q_mode = q.mode; a.rank_tol = rank_tol;
  return launch_with_lds(dsge::smoother_basis_kernel, batch, dsge::KS_THREADS, dsge::ksb_lds_doubles(m, k) * sizeof(double), st, a,
                         "smoother: LDS budget exceeded");
}

int launch_kalman_smoother(const double* T, const double* R, const ShockCov& q, int batch, int m, int k, int T_len,
                           double rank_tol, double* U, double* UT, double* UR, int32_t* rank, const double* a_pred, const double* a_filt,
                           const double* p_pred, const double* p_filt, double* a_s, double* p_s, double* e_s, int full_cov,
                           int32_t* status, hipStream_t st) {
  dsge::KsArgs a{};
  a.T = T; a.R = R; a.Q = q.Q; a.U = U; a.UT = UT; a.UR = UR; a.rank = rank; a.a_pred = a_pred; a.a_filt = a_filt; a.p_pred = p_pred;
  a.p_filt = p_filt; a.a_s = a_s; a.p_s = p_s; a.e_s = e_s; a.status = status; a.batch = batch; a.m = m; a.k = k;
  a.T_len = T_len; a.q_mode = q.mode; a.full_cov = full_cov; a.rank_tol = rank_tol;
  const char* too_large = "smoother: LDS budget exceeded";
  const size_t lds = dsge::ks_lds_doubles(m) * sizeof(double);
  if (lds > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, too_large);  // (before the basis kernel runs)
  if (int rc = launch_smoother_basis(T, R, q, batch, m, k, rank_tol, U, UT, UR, rank, status, st)) return rc;
  if (dsge::ks_u_global(m)) return launch_with_lds(dsge::kalman_smoother_kernel<true>, batch, dsge::KS_THREADS, lds, st, a, too_large);
  return launch_with_lds(dsge::kalman_smoother_kernel<false>, batch, dsge::KS_THREADS, lds, st, a, too_large);
}

size_t smoother_lds_bytes(int m) { return dsge::ks_lds_doubles(m) * sizeof(double); }

// across dated breaks: the draws' status words repeated per segment, the basis of every (draw, segment) on the flattened batch, then
// the backward pass that switches bases at the boundaries
int launch_kalman_smoother_segments(const double* T, const double* R, const ShockCov& q, const int32_t* seg_start, int n_seg, int batch,
                                    int m, int k, int T_len, double rank_tol, double* U, double* UT, double* UR, int32_t* rank,
                                    int32_t* status_flat, const double* a_pred, const double* a_filt, const double* p_pred,
                                    const double* p_filt, double* a_s, double* p_s, double* e_s, int full_cov, int32_t* status,
                                    hipStream_t st) {
  const long long flat = (long long)batch * n_seg, blocks = (flat + 255) / 256;
  hipLaunchKernelGGL(dsge::ks_seg_status_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, status_flat,
                     (const int32_t*)status, flat, n_seg);
  HIP_TRY(hipGetLastError());
  if (int rc = launch_smoother_basis(T, R, q, (int)flat, m, k, rank_tol, U, UT, UR, rank, status_flat, st)) return rc;
  dsge::KsSegArgs a{};
  a.T = T; a.R = R; a.Q = q.Q; a.U = U; a.UT = UT; a.UR = UR; a.rank = rank; a.a_pred = a_pred; a.a_filt = a_filt; a.p_pred = p_pred;
  a.p_filt = p_filt; a.a_s = a_s; a.p_s = p_s; a.e_s = e_s; a.status = status; a.batch = batch; a.m = m; a.k = k;
  a.T_len = T_len; a.q_mode = q.mode; a.full_cov = full_cov; a.rank_tol = rank_tol; a.n_seg = n_seg;
  for (int s = 0; s < DSGE_MAX_SEGMENTS; ++s) a.seg_start[s] = s < n_seg ? seg_start[s] : 0x7fffffff;
  const char* too_large = "segmented smoother: LDS budget exceeded";
  if (dsge::ks_u_global(m))
    return launch_with_lds(dsge::kalman_smoother_kernel<true, true>, batch, dsge::KS_THREADS, smoother_lds_bytes(m), st, a, too_large);
  return launch_with_lds(dsge::kalman_smoother_kernel<false, true>, batch, dsge::KS_THREADS, smoother_lds_bytes(m), st, a, too_large);
}

}  // namespace dsge_host
