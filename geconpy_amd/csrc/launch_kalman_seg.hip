// Launcher of the Kalman likelihood across dated structural breaks (dsge_kalman_seg.hpp): the row copies that bring the caller's
// layouts to the ones the existing sym(R Q R') and Lyapunov launches take, and the filter itself.
#include "dsge_host.hpp"
#include "dsge_kalman_seg.hpp"

namespace dsge_host {

// dst[r][0 .. width-1] = src[(r % mod) * mul][0 .. width-1] for r = 0 .. rows-1 (kseg_rows_kernel)
int launch_segment_rows(double* dst, const double* src, size_t rows, int width, int mod, int mul, hipStream_t st) {
  const size_t n = rows * (size_t)width;
  if (n == 0) return DSGE_SUCCESS;
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(dsge::kseg_rows_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, dst, src,
                     (long long)rows, width, mod, mul);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

size_t kalman_segments_lds_bytes(int m, int p) { return dsge::kseg_lds_doubles(m, p) * sizeof(double); }

int launch_kalman_segments(const double* T, const double* RQR, const double* P0, const double* a0, const double* shift,
                           const ObsModel& o, const int32_t* seg_start, int n_seg, int batch, int m, double* logp, double* ll,
                           double* a_last, double* P_last, int32_t* status, hipStream_t st) {
  dsge::KsegArgs a{};
  a.T = T; a.RQR = RQR; a.P0 = P0; a.a0 = a0; a.shift = shift; a.Z = o.Z; a.d = o.d; a.Hdiag = o.Hdiag; a.y = o.y; a.logp = logp;
  a.ll = ll; a.a_last = a_last; a.P_last = P_last; a.status = status; a.batch = batch; a.m = m; a.p = o.p; a.T_len = o.T_len;
  a.n_seg = n_seg; a.z_batched = o.z_batched; a.d_batched = o.d_batched; a.h_batched = o.h_batched;
  for (int s = 0; s < DSGE_MAX_SEGMENTS; ++s) a.seg_start[s] = s < n_seg ? seg_start[s] : 0x7fffffff;
  a.cv = filter_conv(o.jitter);
  a.missing_fill = o.missing_fill;
  return launch_with_lds(dsge::kalman_seg_kernel<false>, batch, dsge::KSEG_THREADS, kalman_segments_lds_bytes(m, o.p), st, a,
                         "segmented filter: LDS budget exceeded");
}

}  // namespace dsge_host
