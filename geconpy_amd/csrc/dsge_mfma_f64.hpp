// C = op(A) op(B) on the FP64 matrix core (v_mfma_f64_16x16x4_f64) out of zero-padded LDS (or global) images: the product
// helper shared by the smoother (dsge_kalman_smooth.hpp) and the post-solve dynamics kernels (dsge_dynamics.hpp).
#pragma once
#include "dsge_device.hpp"

namespace dsge {

typedef double ks_v4f64 __attribute__((ext_vector_type(4)));
// explicit address spaces for the working pointers: left generic, the fragment loads of ks_gemm compiled to flat loads, which
// count on the VM counter together with the step's prefetch
typedef __attribute__((address_space(3))) double ks_lds;
typedef __attribute__((address_space(1))) double ks_glb;

__host__ __device__ inline int ks_mp(int m) { return (m + 15) & ~15; }
__host__ __device__ inline int ks_ld(int m) { return ks_mp(m) + 2; }
__host__ __device__ inline size_t ks_mat(int m) { return (size_t)ks_mp(m) * ks_ld(m); }  // doubles of one padded image

// ---- C = op(A) op(B) on the FP64 matrix core, operands and result in padded images ---------------------------------------------
// A(i, k) = TA ? A[k lda + i] : A[i lda + k];  B(k, j) = TB ? B[j ldb + k] : B[k ldb + j];  mt x nt output tiles of 16 x 16, K a
// multiple of 4 (the images are zero beyond the data).  Fragments of v_mfma_f64_16x16x4_f64 (dsge_so_gemm.hpp): lane l holds
// A(i = l & 15, k = l >> 4), B(k = l >> 4, j = l & 15) and the results C(4 q + (l >> 4), l & 15), q = 0..3.  The wavefronts
// w0, w0 + nw, ... of the workgroup's four share the tiles round-robin, up to four tiles (independent accumulators) at a time.
template <bool TA, bool TB, class PA, class PB, class Epi>
__device__ __forceinline__ void ks_gemm(PA A, int lda, PB B, int ldb, int mt, int nt, int K, int w0, int nw,
                                        Epi epi) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) - w0;
  if (wave < 0 || wave >= nw) return;
  const int li = lane & 15, lk = lane >> 4, ntile = mt * nt;
  const int sa = TA ? 4 * lda : 4, sb = TB ? 4 : 4 * ldb;
  for (int base = wave; base < ntile; base += 4 * nw) {
    PA pa[4];
    PB pb[4];
    ks_v4f64 acc[4];
    int nv = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = base + q * nw;
      const int tc = t < ntile ? t : base;
      if (t < ntile) nv = q + 1;
      const int ti = tc / nt, tj = tc - ti * nt;
      pa[q] = TA ? A + lk * lda + 16 * ti + li : A + (16 * ti + li) * lda + lk;
      pb[q] = TB ? B + (16 * tj + li) * ldb + lk : B + lk * ldb + 16 * tj + li;
      acc[q] = ks_v4f64{0.0, 0.0, 0.0, 0.0};
    }
    double av[4] = {}, bv[4] = {};  // the fragments of the next four columns are loaded while the current ones multiply
    if (K > 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < nv) {
          av[q] = *pa[q];
          bv[q] = *pb[q];
        }
    }
    for (int k0 = 0; k0 < K; k0 += 4) {
      double an[4] = {}, bn[4] = {};
      if (k0 + 4 < K) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < nv) {
            pa[q] += sa;
            pb[q] += sb;
            an[q] = *pa[q];
            bn[q] = *pb[q];
          }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < nv) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], acc[q], 0, 0, 0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        av[q] = an[q];
        bv[q] = bn[q];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < nv) {
        const int t = base + q * nw, ti = t / nt, tj = t - ti * nt;
#pragma unroll
        for (int e = 0; e < 4; ++e) epi(16 * ti + lk + 4 * e, 16 * tj + li, acc[q][e]);
      }
  }
}

}  // namespace dsge
