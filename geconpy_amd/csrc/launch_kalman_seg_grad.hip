// Launchers of the gradient of the likelihood across dated structural breaks (dsge_kalman_seg_grad.hpp,
// docs/design/segmented_gradient.md): the storing forward pass with logp (kalman_seg_kernel<true>, the instantiation of
// launch_kalman_seg_store.hip with the one output that launcher does not pass on), the reverse sweep, and R_bar / Q_bar.
#include "dsge_host.hpp"
#include "dsge_kalman_seg_grad.hpp"

namespace dsge_host {

size_t kalman_segments_grad_lds_bytes(int m, int p) { return dsge::ksg_lds_doubles(m, p) * sizeof(double); }

int launch_kalman_segments_grad_forward(const double* T, const double* RQR, const double* P0, const double* a0, const double* shift,
                                        const ObsModel& o, const int32_t* seg_start, int n_seg, int batch, int m, double* logp,
                                        double* ap_s, double* af_s, double* pp_s, double* pf_s, int32_t* status, hipStream_t st) {
  dsge::KsegStoreArgs a{};
  a.T = T; a.RQR = RQR; a.P0 = P0; a.a0 = a0; a.shift = shift; a.Z = o.Z; a.d = o.d; a.Hdiag = o.Hdiag; a.y = o.y; a.logp = logp;
  a.status = status; a.batch = batch; a.m = m; a.p = o.p; a.T_len = o.T_len; a.n_seg = n_seg; a.z_batched = o.z_batched;
  a.d_batched = o.d_batched; a.h_batched = o.h_batched;
  for (int s = 0; s < DSGE_MAX_SEGMENTS; ++s) a.seg_start[s] = s < n_seg ? seg_start[s] : 0x7fffffff;
  a.cv = filter_conv(o.jitter);
  a.missing_fill = o.missing_fill;
  a.ap_s = ap_s; a.af_s = af_s; a.pp_s = pp_s; a.pf_s = pf_s;
  return launch_with_lds(dsge::kalman_seg_kernel<true>, batch, dsge::KSEG_THREADS, kalman_segments_lds_bytes(m, o.p), st, a,
                         "segmented gradient: LDS budget exceeded");
}

int launch_kalman_segments_grad(const double* T, const double* shift, const ObsModel& o, const int32_t* seg_start, int n_seg, int batch,
                                int m, int p0_given, const double* ap, const double* af, const double* pp, const double* pf,
                                double* Tbar, double* Gbar, double* Zbar, double* dbar, double* hbar, double* shbar, double* a0bar,
                                double* P0bar, const int32_t* status, hipStream_t st) {
  dsge::KsegGradArgs a{};
  a.T = T; a.shift = shift; a.Z = o.Z; a.d = o.d; a.Hdiag = o.Hdiag; a.y = o.y; a.ap = ap; a.af = af; a.pp = pp; a.pf = pf;
  a.Tbar = Tbar; a.Gbar = Gbar; a.Zbar = Zbar; a.dbar = dbar; a.hbar = hbar; a.shbar = shbar; a.a0bar = a0bar; a.P0bar = P0bar;
  a.status = status; a.batch = batch; a.m = m; a.p = o.p; a.T_len = o.T_len; a.n_seg = n_seg; a.z_batched = o.z_batched;
  a.d_batched = o.d_batched; a.h_batched = o.h_batched; a.p0_given = p0_given;
  for (int s = 0; s < DSGE_MAX_SEGMENTS; ++s) a.seg_start[s] = s < n_seg ? seg_start[s] : 0x7fffffff;
  a.cv = filter_conv(o.jitter);
  a.missing_fill = o.missing_fill;
  return launch_with_lds(dsge::kalman_seg_grad_kernel, batch, dsge::KSG_THREADS, kalman_segments_grad_lds_bytes(m, o.p), st, a,
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
