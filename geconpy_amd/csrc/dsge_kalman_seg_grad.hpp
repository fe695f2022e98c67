// Reverse sweep of the Kalman log-likelihood across DATED STRUCTURAL BREAKS (docs/design/segmented_gradient.md): the gradient of
// dsge_kalman_logp_segments_batched with respect to every entry of T_s, R_s, Q_s, Z_s, d_s, H_s, shift_s, a0 and P0, on the FULL
// model with a general Z.  The forward pass is kalman_seg_kernel<true> (dsge_kalman_seg.hpp), which leaves a_pred, P_pred, a_filt,
// P_filt of every period in library scratch; this kernel walks back over them.  With s = s(t), s' = s(t+1), b = [t+1 ==
// seg_start[s']] and (abar, Pbar) the cotangents of the predicted moments of period t+1:
//   prediction step (t < n-1):
//     Tbar_s' += abar (a_filt[t] + b shift_s')' + 2 Pbar T_s' P_filt[t],   Gbar_s' += Pbar,
//     a+bar = T_s'' abar  (b: shift_bar_s' = a+bar),   P+bar = T_s'' Pbar T_s'
//   update step of period t, on P = P_pred[t], a = a_pred[t] with Z_s, d_s, H_s, the masks of the period and the call's FilterConv
//   (M = P Zm', F = Zm M + Hm + jit_F I, K = M F^-1, e = F^-1 v, P+ = P - K (F + jit_V I) K' + jit_P I; lam = 0 for an empty period):
//     vbar = -lam e + K' a+bar,   Y = P+bar K,   Mbar = a+bar e' - 2 Y - 2 jit_V Y F^-1      (= Kbar F^-1, Kbar = a+bar v' - 2 Y (F + jit_V I))
//     Fbar = -lam/2 (F^-1 - e e') - K' Y - K' Mbar,   Mbar += Zm' Fbar
//     Zbar_s += [observed rows] (-vbar a' + Mbar' P + (Fbar F) K'),   dbar_s -= vbar (masked under mask_d),   hbar_s += w o diag(Fbar)
//     Pbar = sym(P+bar + Mbar Zm),   abar = a+bar - Zm' vbar
//   t = 0:  a0_bar = abar;  P0 given: P0_bar = Pbar;  else S = dlyap(T_0', Pbar) by doubling, Gbar_0 += S, Tbar_0 += 2 S T_0 P0.
// kalman_seg_grad_kernel: one workgroup of 256 threads (4 wavefronts) per draw.  Four zero-padded LDS images (ks_mat) -- Pbar, T_s,
// the image of the period's stored covariance (P_filt[t] for the prediction step, then P_pred[t] for the update) and a work image
// whose space holds the three m x p panels (K, Y, Mbar) during the update.  The three m x m x m products of a step run on the FP64
// matrix core (ks_gemm): Pbar T, T' (Pbar T), (Pbar T) P_filt.  The panels and the p x p block run on the VALU.
// Accumulators: Tbar_s is added to in global memory by the epilogue of the (Pbar T) P_filt product -- ks_gemm gives an entry to the
// same lane every period, so the read-modify-write has one owner and needs neither atomics nor a barrier; Gbar_s, Zbar_s, dbar_s,
// hbar_s are carried in registers by the thread that owns the entry and stored once, at the boundary that closes the segment.  One
// scheme for every m <= 64: at m >= 49 a fifth image does not fit next to the panels, and a second code path for m <= 48 would have
// to be held to the same bits.
// kseg_grad_rq_kernel: per (draw, segment)  R_bar = 2 sym(Gbar) R sym(Q),  Q_bar = R' sym(Gbar) R (its diagonal for a diagonal Q);
// a failed draw gets zeros and logp = -inf.
#pragma once
#include "dsge_kalman_seg.hpp"

namespace dsge {

constexpr int KSG_THREADS = KSEG_THREADS, KSG_LYAP_MAX_DOUBLINGS = 64;

struct KsegGradArgs {
  const double* T;       // [batch][S][m][m]
  const double* shift;   // [batch][S][m] or nullptr
  const double* Z;       // [S][p][m] or [batch][S][p][m]
  const double* d;       // nullptr, [S][p] or [batch][S][p]
  const double* Hdiag;   // nullptr, [S][p] or [batch][S][p]
  const double* y;       // [T_len][p]
  const double *ap, *af, *pp, *pf;  // the stored forward pass: [batch][T_len][m], [batch][T_len][m][m]
  double* Tbar;          // [batch][S][m][m], ZEROED by the launcher: the caller's T_bar or scratch
  double* Gbar;          // [batch][S][m][m] scratch: cotangent of sym(R Q R'), written for every healthy draw
  double* Zbar;          // [batch][S][p][m] or nullptr   (every optional output below: zeroed by the launcher)
  double* dbar;          // [batch][S][p] or nullptr
  double* hbar;          // [batch][S][p] or nullptr
  double* shbar;         // [batch][S][m] or nullptr
  double* a0bar;         // [batch][m] or nullptr
  double* P0bar;         // [batch][m][m] or nullptr; written only when p0_given
  const int32_t* status; // [batch]: a draw with a non-zero word is skipped
  int batch, m, p, T_len, n_seg, z_batched, d_batched, h_batched, p0_given;
  int seg_start[DSGE_MAX_SEGMENTS];
  FilterConv cv;
  double missing_fill;
};

__host__ __device__ inline size_t ksg_work_doubles(int m) {  // the work image, or the three panels where they need more (m <= 48)
  const size_t mat = ks_mat(m), pan = 3 * (size_t)ks_mp(m) * KSEG_PLD;
  return mat > pan ? mat : pan;
}
__host__ __device__ inline size_t ksg_lds_doubles(int m, int p) {
  return 3 * ks_mat(m) + ksg_work_doubles(m) + (size_t)p * kseg_zld(m) + 5 * KSEG_PMAX * KSEG_PMAX + 4 * 64 + 6 * KSEG_PMAX + 8;
}

__device__ __forceinline__ double ksg_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

__global__ __launch_bounds__(KSG_THREADS) void kalman_seg_grad_kernel(KsegGradArgs a) {
  constexpr int NT = KSG_THREADS, PM = KSEG_PMAX, PL = KSEG_PLD, GQ = DSGE_MAX_N * DSGE_MAX_N / NT, ZQ = DSGE_MAX_N * KSEG_PMAX / NT;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, draw = blockIdx.x, m = a.m, p = a.p, mm = m * m, pm = p * m, n = a.T_len, S = a.n_seg;
  if (draw >= a.batch) return;
  if (a.status[draw] != 0) return;  // (every output of such a draw was zeroed by the launcher)
  const int ld = ks_ld(m), mp = ks_mp(m), mt = mp / 16, m4 = ps_r4(m), zl = kseg_zld(m);
  const size_t MAT = ks_mat(m);
  ks_lds* Pb = (ks_lds*)smem;  // Pbar
  ks_lds* Tm = Pb + MAT;
  ks_lds* Pi = Tm + MAT;       // P_filt[t], then P_pred[t]
  ks_lds* W = Pi + MAT;
  ks_lds* pl = W + ksg_work_doubles(m);
  ks_lds* Kg = W;                       // [i][o]: P Zm', then K in place   (the panels live in the work image)
  ks_lds* Yp = Kg + (size_t)mp * PL;    // Y = P+bar K
  ks_lds* Mb = Yp + (size_t)mp * PL;    // Mbar
  ks_lds* Zm = pl; pl += (size_t)p * zl;  // [o][j]
  ks_lds* Fm = pl; pl += PM * PM;
  ks_lds* Lc = pl; pl += PM * PM;       // Cholesky factor of F
  ks_lds* Fi = pl; pl += PM * PM;       // F^-1
  ks_lds* Fb = pl; pl += PM * PM;       // Fbar
  ks_lds* FF = pl; pl += PM * PM;       // Fbar F
  ks_lds* av = pl; pl += 64;            // a_pred[t]
  ks_lds* afs = pl; pl += 64;           // a_filt[t] (+ shift at a boundary)
  ks_lds* ab = pl; pl += 64;            // abar
  ks_lds* apb = pl; pl += 64;           // a+bar
  ks_lds* vv = pl; pl += PM;
  ks_lds* ev = pl; pl += PM;            // F^-1 v
  ks_lds* vb = pl; pl += PM;            // vbar
  ks_lds* dv = pl; pl += PM;
  ks_lds* hv = pl; pl += PM;
  ks_lds* wv = pl; pl += PM;
  ks_lds* red = pl; pl += 8;

  auto stage = [&](int s) {  // T, Z, d, H of segment s (the padding of the T image stays zero); the caller puts the barriers around it
    const size_t ds = (size_t)draw * S + s;
    ps_stage_T(Tm, ld, a.T + ds * mm, m, tid, NT);
    const double* Zg = a.Z + ((a.z_batched ? (size_t)draw * S : 0) + s) * pm;
    for (int idx = tid; idx < pm; idx += NT) {
      const int o = idx / m, j = idx - o * m;
      Zm[o * zl + j] = Zg[idx];
    }
    if (tid < p) {
      dv[tid] = a.d ? a.d[((a.d_batched ? (size_t)draw * S : 0) + s) * p + tid] : 0.0;
      hv[tid] = a.Hdiag ? a.Hdiag[((a.h_batched ? (size_t)draw * S : 0) + s) * p + tid] : 0.0;
    }
  };
  auto load_image = [&](ks_lds* dst, const double* src) {  // [m][m] into the image (its padding is zero and stays zero)
    for (int idx = tid; idx < mm; idx += NT) {
      const int i = idx / m, j = idx - i * m;
      dst[i * ld + j] = src[idx];
    }
  };

  // the accumulators of the segment the sweep is inside, each owned by one thread: entries tid + q NT of Gbar and Zbar, entry tid
  // of dbar and hbar
  double gacc[GQ], zacc[ZQ], dacc = 0.0, hacc = 0.0;
#pragma unroll
  for (int q = 0; q < GQ; ++q) gacc[q] = 0.0;
#pragma unroll
  for (int q = 0; q < ZQ; ++q) zacc[q] = 0.0;
  auto flush = [&](int s) {
    const size_t ds = (size_t)draw * S + s;
#pragma unroll
    for (int q = 0; q < GQ; ++q) {
      const int idx = tid + q * NT;
      if (idx < mm) a.Gbar[ds * mm + idx] = gacc[q];
      gacc[q] = 0.0;
    }
#pragma unroll
    for (int q = 0; q < ZQ; ++q) {
      const int idx = tid + q * NT;
      if (a.Zbar && idx < pm) a.Zbar[ds * pm + idx] = zacc[q];
      zacc[q] = 0.0;
    }
    if (tid < p) {
      if (a.dbar) a.dbar[ds * p + tid] = dacc;
      if (a.hbar) a.hbar[ds * p + tid] = hacc;
    }
    dacc = 0.0;
    hacc = 0.0;
  };

  {
    const size_t total = ksg_lds_doubles(m, p);
    for (size_t idx = tid; idx < total; idx += NT) Pb[idx] = 0.0;
  }
  __syncthreads();
  int seg = S - 1, seg_first = kseg_start(a, seg);
  stage(seg);
  const size_t dn = (size_t)draw * n;

  for (int t = n - 1; t >= 0; --t) {
    if (t < n - 1) {
      // ---- prediction step t -> t + 1, with the matrices of s' = seg (staged)
      const bool bnd = t + 1 == seg_first;
      double* Tb = a.Tbar + ((size_t)draw * S + seg) * mm;
      load_image(Pi, a.pf + (dn + t) * mm);
      if (tid < m) {
        double v = a.af[(dn + t) * m + tid];
        if (bnd && a.shift) v += a.shift[((size_t)draw * S + seg) * m + tid];
        afs[tid] = v;
      }
#pragma unroll
      for (int q = 0; q < GQ; ++q) {
        const int idx = tid + q * NT;
        if (idx < mm) {
          const int i = idx / m, j = idx - i * m;
          gacc[q] += Pb[i * ld + j];
        }
      }
      __syncthreads();
      // W <- Pbar T;  a+bar = T' abar
      ks_gemm<false, false>((const ks_lds*)Pb, ld, (const ks_lds*)Tm, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) { W[i * ld + j] = v; });
      if (tid < m) {
        double acc = 0.0;
#pragma unroll 4
        for (int j = 0; j < m; ++j) acc = fma(Tm[j * ld + tid], ab[j], acc);
        apb[tid] = acc;
      }
      __syncthreads();
      // Tbar += 2 (Pbar T) P_filt + abar afs'  (this lane owns the entry in every period);  Pbar <- T' (Pbar T)
      ks_gemm<false, false>((const ks_lds*)W, ld, (const ks_lds*)Pi, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) {
        if (i < m && j < m) Tb[i * m + j] += fma(2.0, v, ab[i] * afs[j]);
      });
      ks_gemm<true, false>((const ks_lds*)Tm, ld, (const ks_lds*)W, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) { Pb[i * ld + j] = v; });
      if (bnd && a.shbar && tid < m) a.shbar[((size_t)draw * S + seg) * m + tid] = apb[tid];
      __syncthreads();
      if (bnd) {  // (uniform) the sweep leaves segment s': its accumulators are complete; T, Z, d, H of the segment of period t
        flush(seg);
        --seg;
        seg_first = kseg_start(a, seg);
        stage(seg);
      }
    }
    // ---- update step of period t
    load_image(Pi, a.pp + (dn + t) * mm);
    if (tid < m) av[tid] = a.ap[(dn + t) * m + tid];
    int mask = 0;  // (every thread reads the p entries itself: uniform, no barrier)
    for (int o = 0; o < p; ++o) {
      const double yo = a.y[(size_t)t * p + o];
      if (!(yo != yo) && yo != a.missing_fill) mask |= 1 << o;
    }
    const double lam = mask != 0 ? 1.0 : 0.0;
    __syncthreads();
    if (tid < p) {
      const int o = tid;
      const bool on = (mask >> o) & 1;
      double za = 0.0;
      if (on)
        for (int j = 0; j < m; ++j) za = fma(Zm[o * zl + j], av[j], za);
      vv[o] = (on ? a.y[(size_t)t * p + o] : 0.0) - ((on || !a.cv.mask_d) ? dv[o] : 0.0) - za;
    }
    for (int idx = tid; idx < m * p; idx += NT) {  // P Zm'
      const int i = idx / p, o = idx - i * p;
      double acc = 0.0;
      if ((mask >> o) & 1) {
#pragma unroll 4
        for (int j = 0; j < m; ++j) acc = fma(Pi[i * ld + j], Zm[o * zl + j], acc);
      }
      Kg[i * PL + o] = acc;
    }
    __syncthreads();
    if (tid < p * p) {
      const int o = tid / p, o2 = tid - o * p;
      double acc = 0.0;
      if ((mask >> o) & 1)
        for (int j = 0; j < m; ++j) acc = fma(Zm[o * zl + j], Kg[j * PL + o2], acc);
      if (o == o2) acc += (((mask >> o) & 1) ? hv[o] : 0.0) + a.cv.jit_F;
      Fm[o * PM + o2] = acc;
    }
    __syncthreads();
    if (tid == 0) {  // Cholesky factor of F (the forward pass's), e = F^-1 v
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
      for (int o = 0; o < p; ++o) {
        double sv = vv[o];
        for (int r = 0; r < o; ++r) sv -= Lc[o * PM + r] * wv[r];
        wv[o] = sv / Lc[o * PM + o];
      }
      for (int o = p - 1; o >= 0; --o) {
        double sv = wv[o];
        for (int r = o + 1; r < p; ++r) sv -= Lc[r * PM + o] * ev[r];
        ev[o] = sv / Lc[o * PM + o];
      }
    }
    __syncthreads();
    if (tid < m) {  // K row i = F^-1 (P Zm')[i], in place
      const int i = tid;
      for (int o = 0; o < p; ++o) {
        double sv = Kg[i * PL + o];
        for (int r = 0; r < o; ++r) sv -= Lc[o * PM + r] * Kg[i * PL + r];
        Kg[i * PL + o] = sv / Lc[o * PM + o];
      }
      for (int o = p - 1; o >= 0; --o) {
        double sv = Kg[i * PL + o];
        for (int r = o + 1; r < p; ++r) sv -= Lc[r * PM + o] * Kg[i * PL + r];
        Kg[i * PL + o] = sv / Lc[o * PM + o];
      }
    } else if (tid >= 64 && tid < 64 + p) {  // column c of F^-1, in place in the column of Fi
      const int c = tid - 64;
      for (int o = 0; o < p; ++o) {
        double sv = o == c ? 1.0 : 0.0;
        for (int r = 0; r < o; ++r) sv -= Lc[o * PM + r] * Fi[r * PM + c];
        Fi[o * PM + c] = sv / Lc[o * PM + o];
      }
      for (int o = p - 1; o >= 0; --o) {
        double sv = Fi[o * PM + c];
        for (int r = o + 1; r < p; ++r) sv -= Lc[r * PM + o] * Fi[r * PM + c];
        Fi[o * PM + c] = sv / Lc[o * PM + o];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < m * p; idx += NT) {  // Y = P+bar K
      const int i = idx / p, o = idx - i * p;
      double acc = 0.0;
#pragma unroll 4
      for (int j = 0; j < m; ++j) acc = fma(Pb[i * ld + j], Kg[j * PL + o], acc);
      Yp[i * PL + o] = acc;
    }
    if (tid < p) {  // vbar = -lam e + K' a+bar
      double acc = -lam * ev[tid];
      for (int i = 0; i < m; ++i) acc = fma(Kg[i * PL + tid], apb[i], acc);
      vb[tid] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < m * p; idx += NT) {  // Mbar = a+bar e' - 2 Y - 2 jit_V Y F^-1
      const int i = idx / p, o = idx - i * p;
      double yf = 0.0;
      for (int r = 0; r < p; ++r) yf = fma(Yp[i * PL + r], Fi[r * PM + o], yf);
      Mb[i * PL + o] = fma(apb[i], ev[o], -2.0 * Yp[i * PL + o]) - 2.0 * a.cv.jit_V * yf;
    }
    __syncthreads();
    if (tid < p * p) {  // Fbar = -lam/2 (F^-1 - e e') - K' Y - K' Mbar
      const int o = tid / p, o2 = tid - o * p;
      double acc = -0.5 * lam * (Fi[o * PM + o2] - ev[o] * ev[o2]);
      for (int i = 0; i < m; ++i) acc -= Kg[i * PL + o] * (Yp[i * PL + o2] + Mb[i * PL + o2]);
      Fb[o * PM + o2] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < m * p; idx += NT) {  // Mbar += Zm' Fbar
      const int i = idx / p, o = idx - i * p;
      double acc = Mb[i * PL + o];
      for (int r = 0; r < p; ++r)
        if ((mask >> r) & 1) acc = fma(Zm[r * zl + i], Fb[r * PM + o], acc);
      Mb[i * PL + o] = acc;
    }
    if (tid < p * p) {  // Fbar F  (Fbar M' = (Fbar F) K': M itself was overwritten by K)
      const int o = tid / p, o2 = tid - o * p;
      double acc = 0.0;
      for (int r = 0; r < p; ++r) acc = fma(Fb[o * PM + r], Fm[r * PM + o2], acc);
      FF[o * PM + o2] = acc;
    }
    __syncthreads();
    if (tid < p) {
      const bool on = (mask >> tid) & 1;
      if (on) hacc += Fb[tid * PM + tid];
      if (on || !a.cv.mask_d) dacc -= vb[tid];
    }
#pragma unroll
    for (int q = 0; q < ZQ; ++q) {  // Zbar, observed rows: -vbar a' + Mbar' P + (Fbar F) K'
      const int idx = tid + q * NT;
      if (idx < pm) {
        const int o = idx / m, j = idx - o * m;
        if ((mask >> o) & 1) {
          double acc = -vb[o] * av[j];
#pragma unroll 4
          for (int i = 0; i < m; ++i) acc = fma(Mb[i * PL + o], Pi[i * ld + j], acc);
          for (int r = 0; r < p; ++r) acc = fma(FF[o * PM + r], Kg[j * PL + r], acc);
          zacc[q] += acc;
        }
      }
    }
    double pn[GQ];  // Pbar = sym(P+bar + Mbar Zm): read everything, then write
#pragma unroll
    for (int q = 0; q < GQ; ++q) {
      const int idx = tid + q * NT;
      pn[q] = 0.0;
      if (idx < mm) {
        const int i = idx / m, j = idx - i * m;
        double acc = Pb[i * ld + j] + Pb[j * ld + i];
        for (int o = 0; o < p; ++o)
          if ((mask >> o) & 1) acc += Mb[i * PL + o] * Zm[o * zl + j] + Mb[j * PL + o] * Zm[o * zl + i];
        pn[q] = 0.5 * acc;
      }
    }
    if (tid < m) {  // abar = a+bar - Zm' vbar
      double acc = apb[tid];
      for (int o = 0; o < p; ++o)
        if ((mask >> o) & 1) acc -= Zm[o * zl + tid] * vb[o];
      ab[tid] = acc;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < GQ; ++q) {
      const int idx = tid + q * NT;
      if (idx < mm) {
        const int i = idx / m, j = idx - i * m;
        Pb[i * ld + j] = pn[q];
      }
    }
    __syncthreads();
  }

  // ---- t = 0: the initial moments (segment 0 is staged; Pi holds P_pred[0] = P0)
  if (a.a0bar && tid < m) a.a0bar[(size_t)draw * m + tid] = ab[tid];
  if (a.p0_given) {
    if (a.P0bar)
      for (int idx = tid; idx < mm; idx += NT) {
        const int i = idx / m, j = idx - i * m;
        a.P0bar[(size_t)draw * mm + idx] = Pb[i * ld + j];
      }
  } else {
    // S = dlyap(T_0', Pbar) = sum_k (T_0')^k Pbar T_0^k by doubling, in the Pbar image: S += A' (S A), A <- A A, from A = T_0.  The
    // forward launch's stopping rule: the step's increment at most 1e-17 of the largest entry of S, at most 64 doublings.  The cap is
    // not a silent failure: the powers of T_0 are the forward iteration's, which met the same rule on sym(R Q R') within the same cap
    // or set DSGE_ST_LYAP_FAIL -- and a draw with that bit returned at the top of this kernel.
    ks_lds *A = Tm, *A2 = Pi;
    for (int it = 0; it < KSG_LYAP_MAX_DOUBLINGS; ++it) {
      ks_gemm<false, false>((const ks_lds*)Pb, ld, (const ks_lds*)A, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) { W[i * ld + j] = v; });
      __syncthreads();
      double dmax = 0.0, smax = 0.0;
      ks_gemm<true, false>((const ks_lds*)A, ld, (const ks_lds*)W, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) {
        const double sn = Pb[i * ld + j] + v;
        Pb[i * ld + j] = sn;
        dmax = fmax(dmax, fabs(v));
        smax = fmax(smax, fabs(sn));
        if (v != v) dmax = INFINITY;
      });
      ks_gemm<false, false>((const ks_lds*)A, ld, (const ks_lds*)A, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) { A2[i * ld + j] = v; });
      dmax = ksg_wave_max(dmax);
      smax = ksg_wave_max(smax);
      if ((tid & 63) == 0) {
        red[tid >> 6] = dmax;
        red[4 + (tid >> 6)] = smax;
      }
      __syncthreads();
      dmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
      smax = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
      ks_lds* sw = A;
      A = A2;
      A2 = sw;
      __syncthreads();  // (red is written again in the next round)
      if (!(dmax <= 1.797e308) || !(smax < 1e300) || dmax <= 1e-17 * smax) break;
    }
    // Gbar_0 += S;  Tbar_0 += 2 S T_0 P0, with T_0 and P0 staged again over the powers of T_0 (whose padding is zero)
    ps_stage_T(A, ld, a.T + (size_t)draw * S * mm, m, tid, NT);
    load_image(A2, a.pp + dn * mm);
#pragma unroll
    for (int q = 0; q < GQ; ++q) {
      const int idx = tid + q * NT;
      if (idx < mm) {
        const int i = idx / m, j = idx - i * m;
        gacc[q] += Pb[i * ld + j];
      }
    }
    __syncthreads();
    ks_gemm<false, false>((const ks_lds*)Pb, ld, (const ks_lds*)A, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) { W[i * ld + j] = v; });
    __syncthreads();
    double* Tb = a.Tbar + (size_t)draw * S * mm;
    ks_gemm<false, false>((const ks_lds*)W, ld, (const ks_lds*)A2, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) {
      if (i < m && j < m) Tb[i * m + j] += 2.0 * v;
    });
  }
  flush(0);
}

// R_bar, Q_bar of one (draw, segment) from Gbar: one workgroup per problem of the flattened batch * S; Q is a *_BATCHED layout over
// the flattened batch (full: k x k).  A failed draw: zeros, and logp = -inf (written by the workgroup of its segment 0).
struct KsegGradRqArgs {
  const double* Gbar;  // [flat][m][m]
  const double* R;     // [flat][m][k]
  const double* Q;     // [flat][k] or [flat][k][k]
  double* Rbar;        // [flat][m][k] or nullptr
  double* Qbar;        // [flat][k] or [flat][k][k], or nullptr
  double* logp;        // [batch]
  const int32_t* status;
  int flat, n_seg, m, k, q_full;
};

__host__ __device__ inline size_t ksg_rq_lds_doubles(int m, int k) { return (size_t)m * (m + 1) + (size_t)m * k + (size_t)k * k; }

__global__ __launch_bounds__(256) void kseg_grad_rq_kernel(KsegGradRqArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, prob = blockIdx.x, m = a.m, k = a.k, mk = m * k, kk = k * k, gl = m + 1;
  if (prob >= a.flat) return;
  const int draw = prob / a.n_seg;
  const int qw = a.q_full ? kk : k;
  double* Rb = a.Rbar ? a.Rbar + (size_t)prob * mk : nullptr;
  double* Qb = a.Qbar ? a.Qbar + (size_t)prob * qw : nullptr;
  if (a.status[draw] != 0) {
    if (Rb)
      for (int idx = tid; idx < mk; idx += 256) Rb[idx] = 0.0;
    if (Qb)
      for (int idx = tid; idx < qw; idx += 256) Qb[idx] = 0.0;
    if (tid == 0 && prob == draw * a.n_seg) a.logp[draw] = -INFINITY;
    return;
  }
  double* Gs = smem;               // sym(Gbar), row stride m + 1
  double* X = Gs + (size_t)m * gl; // sym(Gbar) R
  double* Qs = X + mk;             // sym(Q) (full)
  const double* Gg = a.Gbar + (size_t)prob * m * m;
  const double* Rg = a.R + (size_t)prob * mk;
  const double* Qg = a.Q + (size_t)prob * qw;
  for (int idx = tid; idx < m * m; idx += 256) {
    const int i = idx / m, j = idx - i * m;
    Gs[i * gl + j] = 0.5 * (Gg[idx] + Gg[j * m + i]);
  }
  if (a.q_full)
    for (int idx = tid; idx < kk; idx += 256) {
      const int c = idx / k, c2 = idx - c * k;
      Qs[idx] = 0.5 * (Qg[idx] + Qg[c2 * k + c]);
    }
  __syncthreads();
  for (int idx = tid; idx < mk; idx += 256) {
    const int i = idx / k, c = idx - i * k;
    double acc = 0.0;
    for (int j = 0; j < m; ++j) acc = fma(Gs[i * gl + j], Rg[j * k + c], acc);
    X[idx] = acc;
  }
  __syncthreads();
  if (Rb)
    for (int idx = tid; idx < mk; idx += 256) {
      const int i = idx / k, c = idx - i * k;
      double acc;
      if (a.q_full) {
        acc = 0.0;
        for (int c2 = 0; c2 < k; ++c2) acc = fma(X[i * k + c2], Qs[c2 * k + c], acc);
      } else acc = X[idx] * Qg[c];
      Rb[idx] = 2.0 * acc;
    }
  if (Qb)
    for (int idx = tid; idx < qw; idx += 256) {
      const int c = a.q_full ? idx / k : idx, c2 = a.q_full ? idx - c * k : idx;
      double acc = 0.0;
      for (int i = 0; i < m; ++i) acc = fma(Rg[i * k + c], X[i * k + c2], acc);
      Qb[idx] = acc;
    }
}

}  // namespace dsge
