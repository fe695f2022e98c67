// SIMULATION SMOOTHER: joint posterior draws of the whole state path and of the structural shocks per parameter draw (Durbin and
// Koopman's mean correction on the stored filter; docs/design/simulation_smoother.md).  Smoothing is affine in the data and its
// gains depend on the covariances only, so with (x+, y+) drawn from the model
//     x~ = x+ + smooth(y - y+),      eps~ = eps+ + smooth_shocks(y - y+)
// is a draw from the joint posterior of the stored filter's model.  Per (draw, path s), n = T_len, 0-based t:
//     x+[-1] = x0+;  x+[t] = T x+[t-1] + R eps+[t]                       (dynamics_propagate_kernel, dsge_dynamics.hpp)
//     y*[t]  = y[t] - Z x+[t] - eta+[t]                                   (a missing entry of y stays missing; never stored)
//     v = y* - d - Zm a*_pred;  a*_filt = a*_pred + (P Zm') F^-1 v;  a*_pred[t+1] = T a*_filt      (simsmooth_forward_kernel)
//     as*[n-1] = a*_filt[n-1];  z = M^-1 U' (as*[t+1] - a*_pred[t+1]);  as*[t] = a*_filt[t] + P_filt[t] (U'T)' z;
//     es*[t+1] = Q (U'R)' z                                               (simsmooth_backward_kernel)
//     x~[t] = x+[t] + as*[t];   eps~[t] = eps+[t] + es*[t] for t >= 1,  eps~[0] = NaN by the smoother's definition
// P_pred, P_filt are those of kalman_outputs_kernel on y itself (they do not depend on data values), U, U'T, U'R and the rank
// those of smoother_basis_kernel, M = sym(U' P_pred[t+1] U): the MEAN half of kalman_smoother_kernel (dsge_kalman_smooth.hpp)
// with up to 16 right-hand sides.
//
// Both kernels: one workgroup of 256 threads per (draw, group of <= 16 paths).  The paths of a group are the columns of
// path-major LDS images X[path][variable] with the row stride == 2 (mod 32) of ks_gemm's fragment loads, zero beyond the data
// (paths >= nc and variables >= m), so every m x m x 16 product is one row of tiles of v_mfma_f64_16x16x4_f64.  A column of such
// a product, a right-hand side of the elimination and every per-path VALU loop read their own path only: a path's numbers do
// not depend on which other paths share its group.  What depends on the draw alone -- P Zm', F and its factor, E = P_pred U,
// M and its elimination -- is done once per step for the whole group.
#pragma once
#include <type_traits>

#include "dsge_postsolve.hpp"  // staging of T, the per-draw slices, the padding rule, the NaN fill (docs/design/dynamics.md)

namespace dsge {

constexpr int SS_THREADS = 256, SS_COLS = 16, SS_PF = 16;  // SS_PF * SS_THREADS >= 64 * 64: a matrix in flight
constexpr int SS_PMAX = 16;
constexpr int SS_ZLD = 18;  // row stride of the [<= 64][16 paths] images of the backward kernel

__host__ __device__ inline bool ss_u_global(int m) { return m > 48; }
__host__ __device__ inline size_t ssf_lds_doubles(int m, int p) {
  return ks_mat(m) + (size_t)m * m + (size_t)p * m + 2 * (size_t)m * SS_PMAX + 2 * SS_PMAX * SS_PMAX +
         3 * (size_t)SS_COLS * ks_ld(m) + SS_COLS * SS_PMAX + 2 * SS_PMAX + 16;
}
__host__ __device__ inline size_t ssb_lds_doubles(int m) {
  return (ss_u_global(m) ? 3 : 6) * ks_mat(m) + 2 * (size_t)SS_COLS * ks_ld(m) + 2 * 64 * SS_ZLD + 2 * 64 + 16;
}

struct SsArgs {
  const double* T;       // [batch][m][m]
  const double* Q;       // layout q_mode (DSGE_Q_*)
  const double* Z;       // [p][m] or [batch][p][m]
  const double* d;       // nullptr, [p] or [batch][p]
  const double* Hdiag;   // nullptr, [p] or [batch][p]
  const double* y;       // [T_len][p]
  const double* U;       // [batch] padded images of smoother_basis_kernel
  const double* UT;
  const double* UR;
  const int32_t* rank;   // [batch]
  const double* p_pred;  // [batch][T_len][m][m]  the forward pass on y (full covariances)
  const double* p_filt;
  const double* xp;      // [batch][n_paths][T_len][m]  x+
  const double* eps;     // [batch | 1][n_paths][T_len][k]  eps+
  const double* eta;     // [batch | 1][n_paths][T_len][p] or nullptr
  long long eps_draw, eta_draw;  // draw strides (0: shared)
  double* a_pred;        // [batch][n_paths][T_len][m]  a*_pred, a*_filt: written by the forward, read by the backward kernel
  double* a_filt;
  double* x_out;         // [batch][n_paths][T_len][m] or nullptr
  double* e_out;         // [batch][n_paths][T_len][k] or nullptr
  int32_t* status;       // [batch] in/out
  int32_t* snap;         // [batch]: the status words as the forward kernel found them (what both kernels decide "failed draw" by:
                         // the backward kernel's groups run in any order, and group 0 of a draw writes its status word)
  int batch, m, k, p, T_len, n_paths, groups, q_mode, z_batched, d_batched, h_batched;
  FilterConv cv;
  double missing_fill;
};

// ---- forward: the filter MEANS of <= 16 transformed data sets over the stored covariance recursion ---------------------------------
__global__ __launch_bounds__(SS_THREADS) void simsmooth_forward_kernel(SsArgs a) {
  constexpr int NT = SS_THREADS, NC = SS_COLS, PM = SS_PMAX;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, m = a.m, p = a.p, mm = m * m, n = a.T_len;
  const int draw = blockIdx.x / a.groups, g = blockIdx.x - draw * a.groups;
  if (draw >= a.batch) return;
  const int32_t stw = a.status[draw];
  if (g == 0 && tid == 0) a.snap[draw] = stw;
  if (stw != 0) return;  // failed solve or filter: the backward kernel fills the outputs with NaN
  const int s0 = g * NC, nc = a.n_paths - s0 < NC ? a.n_paths - s0 : NC;
  const int ld = ks_ld(m), mp = ks_mp(m), mt = mp / 16, m4 = ps_r4(m);
  ks_lds* Tm = (ks_lds*)smem;               // [mp][ld]
  ks_lds* AP = Tm + ks_mat(m);              // [NC][ld]  a*_pred of the step, path-major
  ks_lds* AF = AP + NC * ld;                // [NC][ld]  a*_filt
  ks_lds* XP = AF + NC * ld;                // [NC][ld]  x+ of the step
  ks_lds* P = XP + NC * ld;                 // [m][m]    P_pred[t]
  ks_lds* Zm = P + mm;                      // [p][m]
  ks_lds* PZ = Zm + p * m;                  // [m][PM]
  ks_lds* Kg = PZ + m * PM;                 // [m][PM]
  ks_lds* Fm = Kg + m * PM;                 // [PM][PM]
  ks_lds* Lc = Fm + PM * PM;                // [PM][PM]
  ks_lds* Vv = Lc + PM * PM;                // [NC][PM]  innovations
  ks_lds* dv = Vv + NC * PM;                // [PM]
  ks_lds* hv = dv + PM;                     // [PM]
  const size_t nlds = ssf_lds_doubles(m, p);
  for (size_t idx = tid; idx < nlds; idx += NT) Tm[idx] = 0.0;
  __syncthreads();
  const double* Zg = ps_obs_slice(a.Z, a.z_batched, draw, p * m);
  const double* ppg = a.p_pred + (size_t)draw * n * mm;
  const size_t path_sz = (size_t)n * m, pbase = ((size_t)draw * a.n_paths + s0) * path_sz;
  const double* xpg = a.xp + pbase;
  double* apo = a.a_pred + pbase;
  double* afo = a.a_filt + pbase;
  const double* etg = a.eta ? a.eta + (size_t)draw * a.eta_draw + (size_t)s0 * n * p : nullptr;
  ps_stage_T(Tm, ld, a.T + (size_t)draw * mm, m, tid, NT);
  for (int idx = tid; idx < mm; idx += NT) P[idx] = ppg[idx];
  for (int idx = tid; idx < p * m; idx += NT) Zm[idx] = Zg[idx];
  if (tid < p) {
    dv[tid] = a.d ? ps_obs_slice(a.d, a.d_batched, draw, p)[tid] : 0.0;
    hv[tid] = a.Hdiag ? ps_obs_slice(a.Hdiag, a.h_batched, draw, p)[tid] : 0.0;
  }
  __syncthreads();
  for (int t = 0; t < n; ++t) {
    double ppr[SS_PF] = {};  // P_pred[t + 1], in flight while this step computes
    if (t + 1 < n) {
#pragma unroll
      for (int q = 0; q < SS_PF; ++q) {
        const int idx = tid + q * NT;
        if (idx < mm) ppr[q] = ppg[(size_t)(t + 1) * mm + idx];
      }
    }
    int mask = 0;  // observed entries of y[t] (the same value in every thread)
    for (int o = 0; o < p; ++o) {
      const double yo = a.y[(size_t)t * p + o];
      if (!(yo != yo) && yo != a.missing_fill) mask |= 1 << o;
    }
    // a*_pred[t] out, x+[t] in;  P Zm'
    for (int idx = tid; idx < nc * m; idx += NT) {
      const int j = idx / m, i = idx - j * m;
      apo[(size_t)j * path_sz + (size_t)t * m + i] = AP[j * ld + i];
      XP[j * ld + i] = xpg[(size_t)j * path_sz + (size_t)t * m + i];
    }
    for (int idx = tid; idx < m * p; idx += NT) {
      const int i = idx / p, o = idx - i * p;
      double acc = 0.0;
      if ((mask >> o) & 1)
        for (int j = 0; j < m; ++j) acc = fma(P[i * m + j], Zm[o * m + j], acc);
      PZ[i * PM + o] = acc;
    }
    __syncthreads();
    // v = (y - Z x+ - eta+) - d - Z a*_pred on the observed entries, 0 on the missing ones;  F
    for (int idx = tid; idx < nc * p; idx += NT) {
      const int j = idx / p, o = idx - j * p;
      double v = 0.0;
      if ((mask >> o) & 1) {
        double zx = 0.0, za = 0.0;
        for (int i = 0; i < m; ++i) {
          zx = fma(Zm[o * m + i], XP[j * ld + i], zx);
          za = fma(Zm[o * m + i], AP[j * ld + i], za);
        }
        const double et = etg ? etg[((size_t)j * n + t) * p + o] : 0.0;
        v = ((a.y[(size_t)t * p + o] - zx - et) - dv[o]) - za;
      }
      Vv[j * PM + o] = v;
    }
    if (tid < p * p) {
      const int o = tid / p, o2 = tid - o * p;
      double acc = 0.0;
      if ((mask >> o) & 1)
        for (int j = 0; j < m; ++j) acc = fma(Zm[o * m + j], PZ[j * PM + o2], acc);
      if (o == o2) acc += (((mask >> o) & 1) ? hv[o] : 0.0) + a.cv.jit_F;
      Fm[o * PM + o2] = acc;
    }
    __syncthreads();
    if (tid == 0) {  // Cholesky of F (positive: the filter on y passed this step, or the draw's status would not be 0)
      for (int j = 0; j < p; ++j) {
        double ds = Fm[j * PM + j];
        for (int r = 0; r < j; ++r) ds -= Lc[j * PM + r] * Lc[j * PM + r];
        const double dj = sqrt(ds);
        Lc[j * PM + j] = dj;
        for (int i = j + 1; i < p; ++i) {
          double sv = 0.5 * (Fm[i * PM + j] + Fm[j * PM + i]);
          for (int r = 0; r < j; ++r) sv -= Lc[i * PM + r] * Lc[j * PM + r];
          Lc[i * PM + j] = sv / dj;
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < m; i += NT) {  // K row i = F^-1 (P Zm')[i], solved in place in the thread's own row of Kg
      for (int o = 0; o < p; ++o) {
        double sv = PZ[i * PM + o];
        for (int r = 0; r < o; ++r) sv -= Lc[o * PM + r] * Kg[i * PM + r];
        Kg[i * PM + o] = sv / Lc[o * PM + o];
      }
      for (int o = p - 1; o >= 0; --o) {
        double sv = Kg[i * PM + o];
        for (int r = o + 1; r < p; ++r) sv -= Lc[r * PM + o] * Kg[i * PM + r];
        Kg[i * PM + o] = sv / Lc[o * PM + o];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < nc * m; idx += NT) {  // a*_filt = a*_pred + K v
      const int j = idx / m, i = idx - j * m;
      double acc = AP[j * ld + i];
      for (int o = 0; o < p; ++o) acc = fma(Kg[i * PM + o], Vv[j * PM + o], acc);
      AF[j * ld + i] = acc;
      afo[(size_t)j * path_sz + (size_t)t * m + i] = acc;
    }
    __syncthreads();
    if (t + 1 < n) {  // a*_pred[t + 1] = T a*_filt for the whole group;  P_pred[t + 1]
      ks_gemm<false, true>((const ks_lds*)Tm, ld, (const ks_lds*)AF, ld, mt, 1, m4, 0, 4, [&](int i, int j, double v) {
        if (i < m) AP[j * ld + i] = v;
      });
#pragma unroll
      for (int q = 0; q < SS_PF; ++q) {
        const int idx = tid + q * NT;
        if (idx < mm) P[idx] = ppr[q];
      }
    }
    __syncthreads();
  }
}

// ---- backward: the smoother's mean recursion with <= 16 right-hand sides, outputs with x+ / eps+ added -----------------------------
template <bool UG>
__global__ __launch_bounds__(SS_THREADS) void simsmooth_backward_kernel(SsArgs a) {
  constexpr int NT = SS_THREADS, NC = SS_COLS, ZL = SS_ZLD;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63, m = a.m, k = a.k, mm = m * m, n = a.T_len;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int draw = blockIdx.x / a.groups, g = blockIdx.x - draw * a.groups;
  if (draw >= a.batch) return;
  const int s0 = g * NC, nc = a.n_paths - s0 < NC ? a.n_paths - s0 : NC;
  const size_t path_sz = (size_t)n * m, eps_sz = (size_t)n * k;
  const size_t pbase = ((size_t)draw * a.n_paths + s0) * path_sz, ebase = ((size_t)draw * a.n_paths + s0) * eps_sz;
  double* xo = a.x_out ? a.x_out + pbase : nullptr;
  double* eo = a.e_out ? a.e_out + ebase : nullptr;
  if (a.snap[draw] != 0) {  // failed solve or filter: EVERY path of the draw is NaN
    if (xo) ps_fill_nan(xo, (size_t)nc * path_sz, tid, NT);
    if (eo) ps_fill_nan(eo, (size_t)nc * eps_sz, tid, NT);
    return;
  }
  const int ld = ks_ld(m), mp = ks_mp(m), mt = mp / 16, m4 = ps_r4(m), kt = (k + 15) / 16;
  const size_t MAT = ks_mat(m);
  const int r = a.rank[draw], rt = (r + 15) / 16, r4 = ps_r4(r);
  ks_lds* Pf = (ks_lds*)smem;
  ks_lds* Pp = Pf + MAT;
  ks_lds* W = Pp + MAT;
  ks_lds* AS = W + MAT;          // [NC][ld]  as*[t + 1], path-major
  ks_lds* DL = AS + NC * ld;     // [NC][ld]  as*[t + 1] - a*_pred[t + 1]; later (U'T)' z
  ks_lds* Zr = DL + NC * ld;     // [64][ZL]  U' dl, then z = M^-1 U' dl: row = basis vector, column = path
  ks_lds* RQ = Zr + 64 * ZL;     // [64][ZL]  (U'R)' z: row = shock
  ks_lds* invd = RQ + 64 * ZL;   // [64]      1 / pivot
  ks_lds* qd = invd + 64;        // [64]      diagonal Q
  ks_lds* pl = qd + 64;
  for (size_t idx = tid; idx < (size_t)(pl - Pf); idx += NT) Pf[idx] = 0.0;  // (the padding of every image stays zero)
  typedef typename std::conditional<UG, const ks_glb*, const ks_lds*>::type UPtr;
  UPtr U, UT, UR;
  if constexpr (UG) {
    U = (const ks_glb*)(a.U + (size_t)draw * MAT);
    UT = (const ks_glb*)(a.UT + (size_t)draw * MAT);
    UR = (const ks_glb*)(a.UR + (size_t)draw * MAT);
  } else {
    ks_lds* Ul = pl; pl += MAT;
    ks_lds* UTl = pl; pl += MAT;
    ks_lds* URl = pl; pl += MAT;
    for (size_t idx = tid; idx < MAT; idx += NT) {
      Ul[idx] = a.U[(size_t)draw * MAT + idx];
      UTl[idx] = a.UT[(size_t)draw * MAT + idx];
      URl[idx] = a.UR[(size_t)draw * MAT + idx];
    }
    U = Ul;
    UT = UTl;
    UR = URl;
  }
  bool qf;
  const double* Qg = ps_q_slice(a.Q, a.q_mode, draw, k, &qf);
  const double* xpg = a.xp + pbase;
  const double* apg = a.a_pred + pbase;
  const double* afg = a.a_filt + pbase;
  const double* epg = a.eps + (size_t)draw * a.eps_draw + (size_t)s0 * eps_sz;
  const double* ppg = a.p_pred + (size_t)draw * path_sz * m;
  const double* pfg = a.p_filt + (size_t)draw * path_sz * m;
  __syncthreads();
  if (eo)
    for (int idx = tid; idx < nc * k; idx += NT) eo[(size_t)(idx / k) * eps_sz + idx % k] = NAN;  // eps~[0]
  if (tid < k) qd[tid] = qf ? Qg[tid * k + tid] : Qg[tid];
  {  // t = n - 1: smoothed = filtered; the matrices of step n - 2
    const size_t ol = (size_t)(n - 1) * m;
    if (n >= 2)
      for (int idx = tid; idx < mm; idx += NT) {
        const int i = idx / m, j = idx - i * m;
        Pp[i * ld + j] = ppg[ol * m + idx];
        Pf[i * ld + j] = pfg[(ol - m) * m + idx];
      }
    for (int idx = tid; idx < nc * m; idx += NT) {
      const int j = idx / m, i = idx - j * m;
      const size_t o = (size_t)j * path_sz + ol + i;
      const double v = afg[o];
      AS[j * ld + i] = v;
      if (xo) xo[o] = xpg[o] + v;
    }
  }
  for (int t = n - 2; t >= 0; --t) {
    const size_t ot = (size_t)t * m;
    double pfr[SS_PF] = {}, ppr[SS_PF] = {};  // the matrices of step t - 1, in flight while this step computes
    if (t > 0) {
#pragma unroll
      for (int q = 0; q < SS_PF; ++q) {
        const int idx = tid + q * NT;
        if (idx < mm) {
          pfr[q] = pfg[(ot - m) * m + idx];
          ppr[q] = ppg[ot * m + idx];
        }
      }
    }
    __syncthreads();
    // (1) E = Pp U -> W;  dl of every path
    ks_gemm<false, false>((const ks_lds*)Pp, ld, U, ld, mt, rt, m4, 0, 4, [&](int i, int j, double v) { W[i * ld + j] = v; });
    for (int idx = tid; idx < nc * m; idx += NT) {
      const int j = idx / m, i = idx - j * m;
      DL[j * ld + i] = AS[j * ld + i] - apg[(size_t)j * path_sz + ot + m + i];
    }
    __syncthreads();
    // (2) M = U' E -> Pp;  U' [dl_1 .. dl_S] -> Zr
    ks_gemm<true, false>(U, ld, (const ks_lds*)W, ld, rt, rt, m4, 0, 4, [&](int i, int j, double v) { Pp[i * ld + j] = v; });
    ks_gemm<true, true>(U, ld, (const ks_lds*)DL, ld, rt, 1, m4, 0, 4, [&](int i, int j, double v) { Zr[i * ZL + j] = v; });
    __syncthreads();
    // (3) M <- sym(M)
    for (int i = wave; i < r; i += 4)
      for (int j = lane; j < i; j += 64) {
        const double s = 0.5 * (Pp[i * ld + j] + Pp[j * ld + i]);
        Pp[i * ld + j] = s;
        Pp[j * ld + i] = s;
      }
    // (4) M [z_1 .. z_S] = Zr: the smoother's Gauss-Jordan elimination without pivoting, ONCE for the whole group (pivot k = the
    // square of the Cholesky factor's diagonal entry k); one barrier per pivot, eight rows per wavefront in flight at a time
    for (int kk = 0; kk < r; ++kk) {
      __syncthreads();
      const double dk = Pp[kk * ld + kk];
      if (!(dk > 0.0)) {  // (uniform, and the same verdict in every group of the draw) this step and every earlier one are NaN
        for (int j = 0; j < nc; ++j) {
          if (xo) ps_fill_nan(xo + (size_t)j * path_sz, ot + m, tid, NT);
          if (eo) ps_fill_nan(eo + (size_t)j * eps_sz, (size_t)(t + 2) * k, tid, NT);
        }
        if (g == 0 && tid == 0) a.status[draw] |= DSGE_ST_SMOOTHER_SINGULAR;
        return;
      }
      const double inv = 1.0 / dk;
      if (tid == 0) invd[kk] = inv;
      const int nj = r - kk - 1, ncol = nj + NC;
      for (int ii0 = wave; ii0 < r - 1; ii0 += 32)
        for (int cc = lane; cc < ncol; cc += 64) {
          const bool in_m = cc < nj;
          ks_lds* B = in_m ? Pp : Zr;
          const int lb = in_m ? ld : ZL, off = in_m ? kk + 1 + cc : cc - nj;
          const double pk = B[kk * lb + off];
          double fa[8], v[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int ii = ii0 + 4 * q, i = ii < kk ? ii : ii + 1;
            if (ii < r - 1) {
              fa[q] = Pp[i * ld + kk];
              v[q] = B[i * lb + off];
            }
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int ii = ii0 + 4 * q, i = ii < kk ? ii : ii + 1;
            if (ii < r - 1) B[i * lb + off] = fma(-fa[q] * inv, pk, v[q]);
          }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < r * NC; idx += NT) Zr[(idx / NC) * ZL + idx % NC] *= invd[idx / NC];
    __syncthreads();
    // (5) T' w = (U'T)' z -> DL (path-major);  R' w = (U'R)' z -> RQ      (w = U z itself is never formed)
    ks_gemm<true, false>(UT, ld, (const ks_lds*)Zr, ZL, mt, 1, r4, 0, 4, [&](int i, int j, double v) {
      if (i < m) DL[j * ld + i] = v;
    });
    if (eo) ks_gemm<true, false>(UR, ld, (const ks_lds*)Zr, ZL, kt, 1, r4, 0, 4, [&](int i, int j, double v) { RQ[i * ZL + j] = v; });
    __syncthreads();
    // (6) P_filt[t] (T' w) -> AS;  eps~[t + 1] = eps+[t + 1] + Q (R' w)
    ks_gemm<false, true>((const ks_lds*)Pf, ld, (const ks_lds*)DL, ld, mt, 1, m4, 0, 4, [&](int i, int j, double v) {
      if (i < m) AS[j * ld + i] = v;
    });
    if (eo)
      for (int idx = tid; idx < nc * k; idx += NT) {
        const int j = idx / k, c = idx - j * k;
        double s;
        if (qf) {
          s = 0.0;
          for (int c2 = 0; c2 < k; ++c2) s = fma(Qg[c * k + c2], RQ[c2 * ZL + j], s);
        } else {
          s = qd[c] * RQ[c * ZL + j];
        }
        const size_t o = (size_t)j * eps_sz + (size_t)(t + 1) * k + c;
        eo[o] = epg[o] + s;
      }
    __syncthreads();
    // (7) as*[t] = a*_filt[t] + P_filt[t] T' w;  x~[t] = x+[t] + as*[t];  the matrices of step t - 1
    for (int idx = tid; idx < nc * m; idx += NT) {
      const int j = idx / m, i = idx - j * m;
      const size_t o = (size_t)j * path_sz + ot + i;
      const double v = afg[o] + AS[j * ld + i];
      AS[j * ld + i] = v;
      if (xo) xo[o] = xpg[o] + v;
    }
    if (t > 0) {
#pragma unroll
      for (int q = 0; q < SS_PF; ++q) {
        const int idx = tid + q * NT;
        if (idx < mm) {
          const int i = idx / m, j = idx - i * m;
          Pf[i * ld + j] = pfr[q];
          Pp[i * ld + j] = ppr[q];
        }
      }
    }
  }
}

}  // namespace dsge
