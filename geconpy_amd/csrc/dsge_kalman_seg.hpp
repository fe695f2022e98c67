// Kalman log-likelihood across DATED STRUCTURAL BREAKS (docs/design/segmented_filter.md): the system matrices are piecewise
// constant in time, S <= DSGE_MAX_SEGMENTS segments with the switches at dates the caller knows (seg_start, shared by all draws).
// Period t belongs to segment s(t) = max{s : seg_start[s] <= t}; the matrices of segment s drive the transition INTO every period of
// s and the observation OF every period of s.  The recursion is the full one of dsge_kalman_out.hpp (no steady-state switch, no
// state reduction), under the call's FilterConv:
//     v = ym - d_s - Zm a;  F = Zm P Zm' + Hm + jit_F I;  K = P Zm' F^-1;  a+ = a + K v
//     P+ = P - sym(K (P Zm' + jit_V K)') + jit_P I;    ll_t = -1/2 (c ln 2 pi + ln det F + v' F^-1 v)  (0 if all missing)
//     s' = s(t+1):   a = T_s' (a+ + [t+1 == seg_start[s']] shift_s');   P = sym(T_s' P+ T_s'') + sym(R_s' Q_s' R_s'')
// kalman_seg_kernel: one workgroup of 256 threads (4 wavefronts) per draw.  P, the working matrix W and T_s are zero-padded LDS
// images (ks_mat: 16 ceil(m / 16) rows, row stride == 2 (mod 32) doubles); the two products of sym(T P+ T') run on the FP64 matrix
// core (ks_gemm, v_mfma_f64_16x16x4_f64), the rank-p measurement update on the VALU with the algebra of kalman_outputs_kernel.  At a
// boundary the workgroup re-stages T_s, Z_s, d_s, H_s, switches the sym(R Q R') pointer (global memory: read once per period,
// L2) and adds shift_s to the filtered mean before the product with T_s.  LDS at m = 64, p = 16: three images (101 376 bytes) + Z
// (8 320) + P Zm' and K (8 704 each) + vectors (5 696) = 132 800 of the 160 KiB (kseg_lds_doubles).
#pragma once
#include <type_traits>

#include "dsge_postsolve.hpp"

namespace dsge {

constexpr int KSEG_THREADS = 256, KSEG_PMAX = 16;
constexpr int KSEG_PLD = KSEG_PMAX + 1;  // row stride of P Zm' and K: odd, so the row-per-lane solves read 32 banks pairs apart

struct KsegArgs {
  const double* T;       // [batch][S][m][m]
  const double* RQR;     // [batch][S][m][m] sym(R Q R')
  const double* P0;      // [batch][m][m]
  const double* a0;      // [batch][m] or nullptr (zero)
  const double* shift;   // [batch][S][m] or nullptr
  const double* Z;       // [S][p][m] or [batch][S][p][m]
  const double* d;       // nullptr, [S][p] or [batch][S][p]
  const double* Hdiag;   // nullptr, [S][p] or [batch][S][p]
  const double* y;       // [T_len][p]
  double* logp;          // [batch]
  double* ll;            // [batch][T_len] or nullptr
  double* a_last;        // [batch][m] or nullptr: a_{n-1|n-1}
  double* P_last;        // [batch][m][m] or nullptr: P_{n-1|n-1}
  int32_t* status;       // [batch] in/out
  int batch, m, p, T_len, n_seg, z_batched, d_batched, h_batched;
  int seg_start[DSGE_MAX_SEGMENTS];
  FilterConv cv;
  double missing_fill;
};

// The STORING variant of the kernel (kalman_seg_kernel<true>, the forward pass of the smoother across breaks,
// dsge_kalman_smooth.hpp) also writes the moments of every period: into the smoother's scratch as full matrices, and into the
// caller's arrays (each may be null; covariances as diagonals or full by full_cov).  logp, a_last and P_last may then be null.
struct KsegStoreArgs : KsegArgs {
  double *ap_s, *af_s, *pp_s, *pf_s;  // [batch][T_len][m], [batch][T_len][m][m]: scratch, required
  double *ap_o, *af_o, *pp_o, *pf_o;  // [batch][T_len][m]; [batch][T_len][m] or [batch][T_len][m][m]
  int full_cov;
};

__host__ __device__ inline int kseg_zld(int m) { return m | 1; }  // row stride of Z in LDS (odd)
__host__ __device__ inline size_t kseg_lds_doubles(int m, int p) {
  return 3 * ks_mat(m) + (size_t)p * kseg_zld(m) + 2 * (size_t)ks_mp(m) * KSEG_PLD + 2 * 64 + 2 * KSEG_PMAX * KSEG_PMAX +
         4 * KSEG_PMAX + 8;
}

// first period of segment s, or "never" behind the last one (constant indices only: the list lives in the kernel arguments);
// A: any argument struct with n_seg and seg_start[DSGE_MAX_SEGMENTS] (the filter's, and the reverse sweep's of dsge_kalman_seg_grad.hpp)
template <class A>
__device__ __forceinline__ int kseg_start(const A& a, int s) {
  int v = 0x7fffffff;
#pragma unroll
  for (int q = 0; q < DSGE_MAX_SEGMENTS; ++q)
    if (q == s && q < a.n_seg) v = a.seg_start[q];
  return v;
}

// rows of a source laid out by (row % mod) * mul into consecutive rows of dst: the shared shock covariances [S][w] repeated for
// every draw (mod = S, mul = 1), and segment 0 of every draw gathered out of [batch][S][w] (mod = rows, mul = S)
// (static: this header is included by two translation units, and only launch_kalman_seg.hip launches it)
static __global__ __launch_bounds__(256) void kseg_rows_kernel(double* __restrict__ dst, const double* __restrict__ src, long long rows,
                                                        int width, int mod, int mul) {
  const long long n = rows * width;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
    const long long r = idx / width;
    const int c = (int)(idx - r * width);
    dst[idx] = src[(r % mod) * mul * width + c];
  }
}

// the predicted moments of period t (vector av, LDS image P) into the scratch and, where asked for, the caller's arrays
__device__ __forceinline__ void kseg_store(const KsegStoreArgs& a, int draw, int t, const ks_lds* av, const ks_lds* P, int ld, double* vs,
                                           double* ms, double* vo, double* mo, int tid) {
  const int m = a.m, mm = m * m;
  const size_t o = ((size_t)draw * a.T_len + t) * m;
  if (tid < m) {
    vs[o + tid] = av[tid];
    if (vo) vo[o + tid] = av[tid];
  }
  for (int idx = tid; idx < mm; idx += KSEG_THREADS) {
    const int i = idx / m, j = idx - i * m;
    const double v = P[i * ld + j];
    ms[o * m + idx] = v;
    if (mo) {
      if (a.full_cov) mo[o * m + idx] = v;
      else if (i == j) mo[o + i] = v;
    }
  }
}

template <bool STORE>
__global__ __launch_bounds__(KSEG_THREADS) void kalman_seg_kernel(typename std::conditional<STORE, KsegStoreArgs, KsegArgs>::type a) {
  constexpr int NT = KSEG_THREADS, PM = KSEG_PMAX, PL = KSEG_PLD;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, draw = blockIdx.x, m = a.m, p = a.p, mm = m * m, n = a.T_len, S = a.n_seg;
  if (draw >= a.batch) return;
  double* ll_o = a.ll ? a.ll + (size_t)draw * n : nullptr;
  double* al_o = a.a_last ? a.a_last + (size_t)draw * m : nullptr;
  double* pl_o = a.P_last ? a.P_last + (size_t)draw * mm : nullptr;
  if (a.status[draw] != 0) {  // failed solve or Lyapunov iteration: no filter -- logp = -inf, EVERY other requested output NaN
    if constexpr (STORE) {  // (the scratch of such a draw is never read: the backward pass skips it too)
      const size_t nv = (size_t)n * m, ncv = a.full_cov ? nv * m : nv;
      if (a.ap_o) ps_fill_nan(a.ap_o + (size_t)draw * nv, nv, tid, NT);
      if (a.af_o) ps_fill_nan(a.af_o + (size_t)draw * nv, nv, tid, NT);
      if (a.pp_o) ps_fill_nan(a.pp_o + (size_t)draw * ncv, ncv, tid, NT);
      if (a.pf_o) ps_fill_nan(a.pf_o + (size_t)draw * ncv, ncv, tid, NT);
      if (tid == 0 && a.logp) a.logp[draw] = -INFINITY;
    } else if (tid == 0) a.logp[draw] = -INFINITY;
    if (ll_o) ps_fill_nan(ll_o, n, tid, NT);
    if (al_o) ps_fill_nan(al_o, m, tid, NT);
    if (pl_o) ps_fill_nan(pl_o, mm, tid, NT);
    return;
  }
  const int ld = ks_ld(m), mp = ks_mp(m), mt = mp / 16, m4 = ps_r4(m), zl = kseg_zld(m);
  const size_t MAT = ks_mat(m);
  ks_lds* P = (ks_lds*)smem;
  ks_lds* W = P + MAT;
  ks_lds* Tm = W + MAT;
  ks_lds* pl = Tm + MAT;
  ks_lds* Zm = pl; pl += (size_t)p * zl;   // [o][j]
  ks_lds* PZ = pl; pl += (size_t)mp * PL;  // [i][o]
  ks_lds* Kg = pl; pl += (size_t)mp * PL;
  ks_lds* av = pl; pl += 64;
  ks_lds* af = pl; pl += 64;
  ks_lds* Fm = pl; pl += PM * PM;
  ks_lds* Lc = pl; pl += PM * PM;
  ks_lds* vv = pl; pl += PM;
  ks_lds* dv = pl; pl += PM;
  ks_lds* hv = pl; pl += PM;
  ks_lds* wv = pl; pl += PM;

  // the matrices of segment s into LDS (the padding of the T image stays zero); the caller puts the barriers around it
  auto stage = [&](int s) {
    const size_t ds = (size_t)draw * S + s;
    ps_stage_T(Tm, ld, a.T + ds * mm, m, tid, NT);
    const double* Zg = a.Z + ((a.z_batched ? (size_t)draw * S : 0) + s) * p * m;
    for (int idx = tid; idx < p * m; idx += NT) {
      const int o = idx / m, j = idx - o * m;
      Zm[o * zl + j] = Zg[idx];
    }
    if (tid < p) {
      dv[tid] = a.d ? a.d[((a.d_batched ? (size_t)draw * S : 0) + s) * p + tid] : 0.0;
      hv[tid] = a.Hdiag ? a.Hdiag[((a.h_batched ? (size_t)draw * S : 0) + s) * p + tid] : 0.0;
    }
  };

  for (size_t idx = tid; idx < 3 * MAT; idx += NT) P[idx] = 0.0;
  __syncthreads();
  for (int idx = tid; idx < mm; idx += NT) {
    const int i = idx / m, j = idx - i * m;
    P[i * ld + j] = a.P0[(size_t)draw * mm + idx];
  }
  if (tid < m) av[tid] = a.a0 ? a.a0[(size_t)draw * m + tid] : 0.0;
  stage(0);
  int seg = 0, nxt = kseg_start(a, 1);
  const double* Gg = a.RQR + (size_t)draw * S * mm;
  __syncthreads();

  const double LN2PI = 1.8378770664093453;
  bool finite = true;
  double ll_sum = 0.0;
  for (int t = 0; t < n; ++t) {
    if constexpr (STORE) kseg_store(a, draw, t, (const ks_lds*)av, (const ks_lds*)P, ld, a.ap_s, a.pp_s, a.ap_o, a.pp_o, tid);  // predicted
    int mask = 0;  // (every thread reads the p entries itself: uniform, no barrier)
    for (int o = 0; o < p; ++o) {
      const double yo = a.y[(size_t)t * p + o];
      if (!(yo != yo) && yo != a.missing_fill) mask |= 1 << o;
    }
    // v, P Zm'
    if (tid < p) {
      const int o = tid;
      const bool on = (mask >> o) & 1;
      double za = 0.0;
      if (on)
        for (int j = 0; j < m; ++j) za = fma(Zm[o * zl + j], av[j], za);
      vv[o] = (on ? a.y[(size_t)t * p + o] : 0.0) - ((on || !a.cv.mask_d) ? dv[o] : 0.0) - za;
    }
    for (int idx = tid; idx < m * p; idx += NT) {
      const int i = idx / p, o = idx - i * p;
      double acc = 0.0;
      if ((mask >> o) & 1) {
#pragma unroll 4
        for (int j = 0; j < m; ++j) acc = fma(P[i * ld + j], Zm[o * zl + j], acc);
      }
      PZ[i * PL + o] = acc;
    }
    __syncthreads();
    if (tid < p * p) {
      const int o = tid / p, o2 = tid - o * p;
      double acc = 0.0;
      if ((mask >> o) & 1)
        for (int j = 0; j < m; ++j) acc = fma(Zm[o * zl + j], PZ[j * PL + o2], acc);
      if (o == o2) acc += (((mask >> o) & 1) ? hv[o] : 0.0) + a.cv.jit_F;
      Fm[o * PM + o2] = acc;
    }
    __syncthreads();
    if (tid == 0) {  // Cholesky of F, ln det F, F^-1 v, ll_t
      double ldet = 0.0;
      bool okc = true;
      for (int j = 0; j < p; ++j) {
        double ds = Fm[j * PM + j];
        for (int r = 0; r < j; ++r) ds -= Lc[j * PM + r] * Lc[j * PM + r];
        if (!(ds > 0.0)) okc = false;
        const double dj = sqrt(ds);
        Lc[j * PM + j] = dj;
        ldet += 2.0 * log(dj);
        for (int i = j + 1; i < p; ++i) {
          double sv = 0.5 * (Fm[i * PM + j] + Fm[j * PM + i]);
          for (int r = 0; r < j; ++r) sv -= Lc[i * PM + r] * Lc[j * PM + r];
          Lc[i * PM + j] = sv / dj;
        }
      }
      double quad = 0.0;
      for (int o = 0; o < p; ++o) {
        double sv = vv[o];
        for (int r = 0; r < o; ++r) sv -= Lc[o * PM + r] * wv[r];
        const double w = sv / Lc[o * PM + o];
        wv[o] = w;
        quad = fma(w, w, quad);
      }
      const double l = (mask != 0) ? -0.5 * (a.cv.ll_terms_step(__popc(mask), p) * LN2PI + ldet + quad) : 0.0;
      if (ll_o) ll_o[t] = l;
      ll_sum += l;
      if (!okc || !(l == l)) finite = false;
    }
    __syncthreads();
    if (tid < m) {  // K row i = F^-1 (P Zm')[i], solved in place in the row of Kg; a+ = a + K v
      const int i = tid;
      for (int o = 0; o < p; ++o) {
        double sv = PZ[i * PL + o];
        for (int r = 0; r < o; ++r) sv -= Lc[o * PM + r] * Kg[i * PL + r];
        Kg[i * PL + o] = sv / Lc[o * PM + o];
      }
      for (int o = p - 1; o >= 0; --o) {
        double sv = Kg[i * PL + o];
        for (int r = o + 1; r < p; ++r) sv -= Lc[r * PM + o] * Kg[i * PL + r];
        Kg[i * PL + o] = sv / Lc[o * PM + o];
      }
      double acc = av[i];
      for (int o = 0; o < p; ++o) acc = fma(Kg[i * PL + o], vv[o], acc);
      af[i] = acc;
      if constexpr (STORE) {  // (before a boundary adds shift: a_filt is in the coordinates of the period's own segment)
        const size_t o = ((size_t)draw * n + t) * m + i;
        a.af_s[o] = acc;
        if (a.af_o) a.af_o[o] = acc;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < mm; idx += NT) {  // P+ -> W
      const int i = idx / m, j = idx - i * m;
      double acc = 0.0;
      for (int o = 0; o < p; ++o) {
        const double ki = Kg[i * PL + o], kj = Kg[j * PL + o];
        acc = fma(ki, fma(a.cv.jit_V, kj, PZ[j * PL + o]), acc);
        acc = fma(kj, fma(a.cv.jit_V, ki, PZ[i * PL + o]), acc);
      }
      const double pf = P[i * ld + j] - 0.5 * acc + (i == j ? a.cv.jit_P : 0.0);
      W[i * ld + j] = pf;
      if constexpr (STORE) {
        const size_t o = ((size_t)draw * n + t) * m;
        a.pf_s[o * m + idx] = pf;
        if (a.pf_o) {
          if (a.full_cov) a.pf_o[o * m + idx] = pf;
          else if (i == j) a.pf_o[o + i] = pf;
        }
      }
    }
    if (t == n - 1) {  // the filtered moments of the last period: what dsge_forecast_batched takes as a0, P0
      __syncthreads();
      if (al_o && tid < m) al_o[tid] = af[tid];
      if (pl_o)
        for (int idx = tid; idx < mm; idx += NT) {
          const int i = idx / m, j = idx - i * m;
          pl_o[idx] = W[i * ld + j];
        }
      break;
    }
    // prediction into t + 1: a = T a+,  P = sym(T P+ T') + sym(R Q R'), with the matrices of the segment of t + 1
    if (t + 1 == nxt) {  // (uniform) a boundary: T, Z, d, H of the new segment; nobody reads the old ones any more
      ++seg;
      nxt = kseg_start(a, seg + 1);
      Gg = a.RQR + ((size_t)draw * S + seg) * mm;
      stage(seg);
      if (a.shift && tid < m) af[tid] += a.shift[((size_t)draw * S + seg) * m + tid];  // (af[tid]: this thread's own entry)
    }
    __syncthreads();
    if (tid < m) {
      double acc = 0.0;
#pragma unroll 4
      for (int j = 0; j < m; ++j) acc = fma(Tm[tid * ld + j], af[j], acc);
      av[tid] = acc;
    }
    // P <- P+ T'  (P is free: its last reader was the P+ pass)
    ks_gemm<false, true>((const ks_lds*)W, ld, (const ks_lds*)Tm, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) { P[i * ld + j] = v; });
    __syncthreads();
    // W <- T (P+ T')
    ks_gemm<false, false>((const ks_lds*)Tm, ld, (const ks_lds*)P, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) { W[i * ld + j] = v; });
    __syncthreads();
    for (int idx = tid; idx < mm; idx += NT) {
      const int i = idx / m, j = idx - i * m;
      P[i * ld + j] = 0.5 * (W[i * ld + j] + W[j * ld + i]) + 0.5 * (Gg[idx] + Gg[(size_t)j * m + i]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (!STORE || a.logp) a.logp[draw] = ll_sum;
    if (!finite || !((ll_sum == ll_sum) && (fabs(ll_sum) < 1.797e308))) a.status[draw] |= DSGE_ST_FILTER_NONFINITE;
  }
}

}  // namespace dsge
