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

int launch_kalman_segments(const SegmentedProblem& s, const double* RQR, const double* P0, double* logp, double* ll, double* a_last,
                           double* P_last, int32_t* status, hipStream_t st) {
  dsge::KsegArgs a{};
  fill_segment_args(a, s);
  a.RQR = RQR; a.P0 = P0; a.a0 = s.a0; a.logp = logp; a.ll = ll; a.a_last = a_last; a.P_last = P_last; a.status = status;
  return launch_with_lds(dsge::kalman_seg_kernel<false>, s.batch, dsge::KSEG_THREADS, kalman_segments_lds_bytes(s.m, s.obs.p), st, a,
                         "segmented filter: LDS budget exceeded");
}

}  // namespace dsge_host
