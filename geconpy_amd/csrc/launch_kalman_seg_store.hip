// Launcher of the STORING instantiation of the filter across dated structural breaks (kalman_seg_kernel<true>, dsge_kalman_seg.hpp):
// the forward pass of the smoother across breaks (docs/design/segmented_smoother.md).  A translation unit of its own, so that
// launch_kalman_seg.hip holds the likelihood's instantiation alone.
#include "dsge_host.hpp"
#include "dsge_kalman_seg.hpp"

namespace dsge_host {

int launch_kalman_segments_store(const double* T, const double* RQR, const double* P0, const double* a0, const double* shift,
                                 const ObsModel& o, const int32_t* seg_start, int n_seg, int batch, int m, double* ll, double* ap_s,
                                 double* af_s, double* pp_s, double* pf_s, double* ap_o, double* af_o, double* pp_o, double* pf_o,
                                 int full_cov, int32_t* status, hipStream_t st) {
  dsge::KsegStoreArgs a{};
  a.T = T; a.RQR = RQR; a.P0 = P0; a.a0 = a0; a.shift = shift; a.Z = o.Z; a.d = o.d; a.Hdiag = o.Hdiag; a.y = o.y; a.ll = ll;
  a.status = status; a.batch = batch; a.m = m; a.p = o.p; a.T_len = o.T_len; a.n_seg = n_seg; a.z_batched = o.z_batched;
  a.d_batched = o.d_batched; a.h_batched = o.h_batched;
  for (int s = 0; s < DSGE_MAX_SEGMENTS; ++s) a.seg_start[s] = s < n_seg ? seg_start[s] : 0x7fffffff;
  a.cv = filter_conv(o.jitter);
  a.missing_fill = o.missing_fill;
  a.ap_s = ap_s; a.af_s = af_s; a.pp_s = pp_s; a.pf_s = pf_s; a.ap_o = ap_o; a.af_o = af_o; a.pp_o = pp_o; a.pf_o = pf_o;
  a.full_cov = full_cov;
  return launch_with_lds(dsge::kalman_seg_kernel<true>, batch, dsge::KSEG_THREADS, kalman_segments_lds_bytes(m, o.p), st, a,
                         "segmented smoother: LDS budget exceeded");
}

}  // namespace dsge_host
