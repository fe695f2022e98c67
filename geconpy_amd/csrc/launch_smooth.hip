// Launcher of the fixed-interval smoother (dsge_kalman_smooth.hpp): basis of range(P_pred) per draw, then the backward pass.
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
  int rc;
  const size_t lds_b = dsge::ksb_lds_doubles(m, k) * sizeof(double);
  if (lds_b > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, "smoother: LDS budget exceeded");
  if ((rc = set_lds(dsge::smoother_basis_kernel, lds_b))) return rc;
  hipLaunchKernelGGL(dsge::smoother_basis_kernel, dim3(batch), dim3(dsge::KS_THREADS), lds_b, st, a);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

int launch_kalman_smoother(const double* T, const double* R, const ShockCov& q, int batch, int m, int k, int T_len,
                           double rank_tol, double* U, double* UT, double* UR, int32_t* rank, const double* a_pred, const double* a_filt,
                           const double* p_pred, const double* p_filt, double* a_s, double* p_s, double* e_s, int full_cov,
                           int32_t* status, hipStream_t st) {
  dsge::KsArgs a{};
  a.T = T; a.R = R; a.Q = q.Q; a.U = U; a.UT = UT; a.UR = UR; a.rank = rank; a.a_pred = a_pred; a.a_filt = a_filt; a.p_pred = p_pred;
  a.p_filt = p_filt; a.a_s = a_s; a.p_s = p_s; a.e_s = e_s; a.status = status; a.batch = batch; a.m = m; a.k = k;
  a.T_len = T_len; a.q_mode = q.mode; a.full_cov = full_cov; a.rank_tol = rank_tol;
  int rc;
  const size_t lds = dsge::ks_lds_doubles(m) * sizeof(double);
  if (lds > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, "smoother: LDS budget exceeded");
  if ((rc = launch_smoother_basis(T, R, q, batch, m, k, rank_tol, U, UT, UR, rank, status, st))) return rc;
  if (dsge::ks_u_global(m)) {
    if ((rc = set_lds(dsge::kalman_smoother_kernel<true>, lds))) return rc;
    hipLaunchKernelGGL(dsge::kalman_smoother_kernel<true>, dim3(batch), dim3(dsge::KS_THREADS), lds, st, a);
  } else {
    if ((rc = set_lds(dsge::kalman_smoother_kernel<false>, lds))) return rc;
    hipLaunchKernelGGL(dsge::kalman_smoother_kernel<false>, dim3(batch), dim3(dsge::KS_THREADS), lds, st, a);
  }
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

}  // namespace dsge_host
