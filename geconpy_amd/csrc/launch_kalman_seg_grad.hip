// Launchers of the gradient of the likelihood across dated structural breaks (dsge_kalman_seg_grad.hpp,
// docs/design/segmented_gradient.md): the reverse sweep over the stored forward pass (launch_kalman_seg_store.hip), and R_bar / Q_bar.
#include "dsge_host.hpp"
#include "dsge_kalman_seg_grad.hpp"

namespace dsge_host {

size_t kalman_segments_grad_lds_bytes(int m, int p) { return dsge::ksg_lds_doubles(m, p) * sizeof(double); }

int launch_kalman_segments_grad(const SegmentedProblem& s, const double* ap, const double* af, const double* pp, const double* pf,
                                double* Tbar, double* Gbar, double* Zbar, double* dbar, double* hbar, double* shbar, double* a0bar,
                                double* P0bar, const int32_t* status, hipStream_t st) {
  dsge::KsegGradArgs a{};
  fill_segment_args(a, s);
  a.ap = ap; a.af = af; a.pp = pp; a.pf = pf;
  a.Tbar = Tbar; a.Gbar = Gbar; a.Zbar = Zbar; a.dbar = dbar; a.hbar = hbar; a.shbar = shbar; a.a0bar = a0bar; a.P0bar = P0bar;
  a.status = status; a.p0_given = s.P0 != nullptr;
  return launch_with_lds(dsge::kalman_seg_grad_kernel, s.batch, dsge::KSG_THREADS, kalman_segments_grad_lds_bytes(s.m, s.obs.p), st, a,
                         "segmented gradient: LDS budget exceeded");
}

int launch_kalman_segments_grad_rq(const double* Gbar, const double* R, const ShockCov& q, int flat, int n_seg, int m, int k,
                                   double* Rbar, double* Qbar, double* logp, const int32_t* status, hipStream_t st) {
  dsge::KsegGradRqArgs a{};
  a.Gbar = Gbar; a.R = R; a.Q = q.Q; a.Rbar = Rbar; a.Qbar = Qbar; a.logp = logp; a.status = status; a.flat = flat; a.n_seg = n_seg;
  a.m = m; a.k = k; a.q_full = q.diag() ? 0 : 1;
  return launch_with_lds(dsge::kseg_grad_rq_kernel, flat, 256, dsge::ksg_rq_lds_doubles(m, k) * sizeof(double), st, a,
                         "segmented gradient: LDS budget exceeded");
}

}  // namespace dsge_host
