// The pieces the post-solve kernels share: free inline functions only.  A kernel calls one only where the compiler's code for it
// stays what it was or was measured no slower; those sites and the ones that keep their own lines: docs/design/dynamics.md.
#pragma once
#include "dsge_mfma_f64.hpp"

namespace dsge {

// ---- padding and stride --------------------------------------------------------------------------------------------------------
__host__ __device__ inline int ps_r4(int x) { return (x + 3) & ~3; }
// row stride of the [T | R] and [x ; e] images: the smallest value == 2 (mod 32) that holds m4 + k4 (+ extra) doubles
__host__ __device__ inline int ps_ld(int m, int k, int extra = 0) { return (ps_r4(m) + ps_r4(k) + extra + 29) / 32 * 32 + 2; }

// ---- staging (into images zeroed before) ------------------------------------------------------------------------------------------
// T [m][m] into columns 0 .. m-1 of the image Tm with row stride ld
__device__ __forceinline__ void ps_stage_T(ks_lds* Tm, int ld, const double* Tg, int m, int tid, int NT) {
  for (int idx = tid; idx < m * m; idx += NT) {
    const int i = idx / m, j = idx - i * m;
    Tm[i * ld + j] = Tg[idx];
  }
}
// [T | R]: T as above, R [m][k] from column m4 on
__device__ __forceinline__ void ps_stage_TR(ks_lds* TR, int ld, int m4, const double* Tg, const double* Rg, int m, int k, int tid,
                                            int NT) {
  ps_stage_T(TR, ld, Tg, m, tid, NT);
  for (int idx = tid; idx < m * k; idx += NT) {
    const int i = idx / k, c = idx - i * k;
    TR[i * ld + m4 + c] = Rg[idx];
  }
}

// ---- the product step ------------------------------------------------------------------------------------------------------------
// nxt[j][0 .. m4-1] = [T | R] cur[j][0 .. K-1] for the 16 columns j of the path-major images; columns behind m4 of nxt: the caller's
__device__ __forceinline__ void ps_step(const ks_lds* TR, const ks_lds* cur, ks_lds* nxt, int ld, int mt, int K, int m4) {
  ks_gemm<false, true>(TR, ld, cur, ld, mt, 1, K, 0, 4, [&](int i, int j, double v) {
    if (i < m4) nxt[j * ld + i] = v;
  });
}
__device__ __forceinline__ void ps_swap(ks_lds*& cur, ks_lds*& nxt) {
  ks_lds* sw = cur;
  cur = nxt;
  nxt = sw;
}

// ---- per-draw slices ---------------------------------------------------------------------------------------------------------------
// the draw's shock covariance in layout q_mode (DSGE_Q_*): k variances, or with *full a k x k matrix
__device__ __forceinline__ const double* ps_q_slice(const double* Q, int q_mode, int draw, int k, bool* full) {
  const bool qb = q_mode == DSGE_Q_DIAG_BATCHED || q_mode == DSGE_Q_FULL_BATCHED;
  const bool qf = q_mode == DSGE_Q_FULL_SHARED || q_mode == DSGE_Q_FULL_BATCHED;
  *full = qf;
  return Q + (qb ? (size_t)draw * (qf ? k * k : k) : 0);
}
// Z, d or Hdiag of the draw: `count` doubles per draw when batched, else shared
__device__ __forceinline__ const double* ps_obs_slice(const double* ptr, int batched, int draw, int count) {
  return ptr + (batched ? (size_t)draw * count : 0);
}

// ---- NaN fill of a failed draw -----------------------------------------------------------------------------------------------------
// `out` is not null: a kernel tests an optional output itself, `if (xo) ps_fill_nan(xo, ...)`
__device__ __forceinline__ void ps_fill_nan(double* out, size_t count, int tid, int NT) {
  for (size_t i = tid; i < count; i += NT) out[i] = NAN;
}

}  // namespace dsge
