// Launcher of the STORING instantiation of the filter across dated structural breaks (kalman_seg_kernel<true>, dsge_kalman_seg.hpp):
// the forward pass of the smoother (docs/design/segmented_smoother.md) and of the gradient (docs/design/segmented_gradient.md)
// across breaks.  A translation unit of its own, so that launch_kalman_seg.hip holds the likelihood's instantiation alone.
#include "dsge_host.hpp"
#include "dsge_kalman_seg.hpp"

namespace dsge_host {

// (the entries refuse an LDS image beyond the budget under their own names before they come here)
int launch_kalman_segments_store(const SegmentedProblem& s, const double* RQR, const double* P0, double* logp, double* ll,
                                 double* ap_s, double* af_s, double* pp_s, double* pf_s, double* ap_o, double* af_o, double* pp_o,
                                 double* pf_o, int full_cov, int32_t* status, hipStream_t st) {
  dsge::KsegStoreArgs a{};
  fill_segment_args(a, s);
  a.RQR = RQR; a.P0 = P0; a.a0 = s.a0; a.logp = logp; a.ll = ll; a.status = status;
  a.ap_s = ap_s; a.af_s = af_s; a.pp_s = pp_s; a.pf_s = pf_s; a.ap_o = ap_o; a.af_o = af_o; a.pp_o = pp_o; a.pf_o = pf_o;
  a.full_cov = full_cov;
  return launch_with_lds(dsge::kalman_seg_kernel<true>, s.batch, dsge::KSEG_THREADS, kalman_segments_lds_bytes(s.m, s.obs.p), st, a,
                         "segmented filter: LDS budget exceeded");
}

}  // namespace dsge_host
