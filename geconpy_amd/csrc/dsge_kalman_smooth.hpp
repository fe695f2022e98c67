// Fixed-interval (Rauch-Tung-Striebel) SMOOTHER on the stored outputs of the "standard" filter (dsge_kalman_out.hpp): the third
// thing `save_kalman_filter_outputs_in_idata` keeps per draw (gEconpy/model/statespace.py:1145, 1151-1157 -> pymc_extras'
// smoother graph; plotted by gEconpy/plotting.py:1791-1835 as "smoothed"), plus the smoothed structural shocks, which upstream
// does not have.  With n = T_len, 0-based t and the filter's a_pred, P_pred, a_filt, P_filt under the call's FilterConv:
//     as[n-1] = a_filt[n-1];  V[n-1] = P_filt[n-1]
//     t = n-2 .. 0:   Pp = P_pred[t+1]                     (= sym(T P_filt[t] T') + sym(R Q R'), from the forward pass)
//                     w  = Pp^+ (as[t+1] - a_pred[t+1])
//                     as[t]    = a_filt[t] + P_filt[t] T' w
//                     eps[t+1] = Q R' w                    (the shock that moves x_t to x_{t+1}; eps[0] = NaN BY DEFINITION: the
//                                                           period-0 innovation is confounded with the pre-sample state)
//                     G = P_filt[t] T' Pp^+;   V[t] = P_filt[t] + sym(G (V[t+1] - Pp) G')
// Pp is singular for every DSGE model (T has zero columns); upstream takes pinv(Pp, hermitian=True).  Here the pseudo-inverse
// comes from the RANGE of Pp, which is fixed per draw: range(Pp) = range(T) + range(R_J), J = {j : Q_jj > 0} -- under TWO
// ASSUMPTIONS: P_filt is positive definite (jitter_on_P guarantees it) and Q_JJ is positive definite.  smoother_basis_kernel
// builds once per draw an orthonormal basis U (m x r) of [T | R_J] (pivoted modified Gram-Schmidt, every column orthogonalised
// twice; rank by |R_jj| > rank_tol |R_00|), U'T and U'R; per step M = sym(U' Pp U) (r x r) and Pp^+ x = U M^-1 U' x.  A
// non-positive pivot of M (possible only with jitter_on_P off) gives the draw DSGE_ST_SMOOTHER_SINGULAR and NaN for that step and
// all earlier ones.  No eigendecomposition, and NOT the Durbin-Koopman r_t / N_t recursion: with jitter on P_filt and F the
// stored filter is not the exact filter of any model, and that recursion differs from this one by 1e-4 (docs/design/smoother.md).
//
// kalman_smoother_kernel: one workgroup of 256 threads (4 wavefronts) per draw.  V[t+1] stays in LDS; P_filt[t] and P_pred[t+1]
// of the NEXT step are loaded into registers while this step computes.  Matrix products per step, all on the FP64 matrix core
// (v_mfma_f64_16x16x4_f64, operands in LDS images of 16 ceil(m / 16) rows with a row stride == 2 (mod 32) doubles, zero padded):
//     E = Pp U;  M = U' E;  C = (U'T) P_filt  [= U' (T P_filt): U'T is per draw, so the square product T P_filt is never formed];
//     G' = U (M^-1 C);  F = (V - Pp) G';  S = G F        -- the last four only when a covariance output is requested.
// The r x r system M [X | z] = [C | U' dl] is eliminated on the VALU by the whole workgroup (pivots = squared Cholesky diagonal),
// the matrix-vector products run there too; w = U z itself is never formed: T' w = (U'T)' z, R' w = (U'R)' z.  m <= 48: U, U'T
// and U'R in LDS (seven images, 131 KiB at m = 33..48); m = 49..64: they are read from global memory (L2), the four working
// matrices take 132 of the 160 KiB.
#pragma once
#include <type_traits>

#include "dsge_postsolve.hpp"  // the slice of Q, the padding rule and the NaN fill (docs/design/dynamics.md, "the shared pieces")

namespace dsge {

constexpr int KS_THREADS = 256, KS_PF = 16;  // KS_PF * KS_THREADS >= 64 * 64: a matrix in flight, KS_PF doubles per thread

__host__ __device__ inline bool ks_u_global(int m) { return m > 48; }
__host__ __device__ inline size_t ks_lds_doubles(int m) { return (ks_u_global(m) ? 4 : 7) * ks_mat(m) + 9 * 64 + 16; }
__host__ __device__ inline size_t ksb_lds_doubles(int m, int k) {
  return (size_t)m * (m + k + 1) + (size_t)m * (m + 1) + (size_t)(m + k) + 3 * (size_t)m + 16;
}

struct KsArgs {
  const double* T;       // [batch][m][m]
  const double* R;       // [batch][m][k]
  const double* Q;       // layout q_mode (DSGE_Q_*)
  double* U;             // [batch] padded images (ks_mat doubles): U[i][a], basis of range(Pp); written by the basis kernel
  double* UT;            // [batch] padded images: (U'T)[a][j]
  double* UR;            // [batch] padded images: (U'R)[a][j]
  int32_t* rank;         // [batch]
  const double* a_pred;  // [batch][T_len][m]      the forward pass (full covariances)
  const double* a_filt;
  const double* p_pred;  // [batch][T_len][m][m]
  const double* p_filt;
  double* a_s;           // [batch][T_len][m] or nullptr
  double* p_s;           // [batch][T_len][m] (diagonals) or [batch][T_len][m][m] (full_cov) or nullptr
  double* e_s;           // [batch][T_len][k] or nullptr
  int32_t* status;       // [batch] in/out
  int batch, m, k, T_len, q_mode, full_cov;
  double rank_tol;
};

// ACROSS DATED BREAKS (kalman_smoother_kernel<UG, true>; docs/design/segmented_smoother.md): the stored forward pass is that of
// kalman_seg_kernel<true> (dsge_kalman_seg.hpp) and step t uses the matrices of s' = s(t+1).  The range of P_pred[t+1] is fixed per
// (draw, segment), so U, UT, UR are [batch][S] images, rank is [batch][S] and Q is per (draw, segment) (a *_BATCHED layout over
// batch * S): the basis kernel runs unchanged on the flattened batch.  Walking back over a boundary (t + 1 == seg_start[s']) the
// workgroup re-stages the three LDS images (m <= 48) or moves its three pointers (m >= 49), and reads r and the diagonal of Q anew.
struct KsSegArgs : KsArgs {
  int n_seg;
  int seg_start[DSGE_MAX_SEGMENTS];
};

// first period of segment s (constant indices only: the list lives in the kernel arguments)
__device__ __forceinline__ int ks_seg_start(const KsSegArgs& a, int s) {
  int v = 0;
#pragma unroll
  for (int q = 0; q < DSGE_MAX_SEGMENTS; ++q)
    if (q == s) v = a.seg_start[q];
  return v;
}

// the draw's status word repeated for each of its segments: what the basis kernel reads on the flattened batch
__global__ __launch_bounds__(256) void ks_seg_status_kernel(int32_t* __restrict__ dst, const int32_t* __restrict__ src, long long flat,
                                                            int n_seg) {
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < flat; idx += (long long)gridDim.x * 256) dst[idx] = src[idx / n_seg];
}

// ---- basis of [T | R_J] and U'T, once per draw ---------------------------------------------------------------------------------
__global__ __launch_bounds__(KS_THREADS) void smoother_basis_kernel(KsArgs a) {
  constexpr int NT = KS_THREADS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63, draw = blockIdx.x, m = a.m, k = a.k, nc = m + k, la = nc + 1, lu = m + 1;
  if (draw >= a.batch || a.status[draw] != 0) return;
  double* A = smem;                    // [m][la]: the columns still to be orthogonalised
  double* Uq = A + (size_t)m * la;     // [m][lu]
  double* cn = Uq + (size_t)m * lu;    // [nc]
  double* qv = cn + nc;                // [m]
  double* hv = qv + m;                 // [m]
  double* pvs = hv + m;                // [2]: pivot norm^2, pivot index
  const double* Tg = a.T + (size_t)draw * m * m;
  const double* Rg = a.R + (size_t)draw * m * k;
  bool qf;
  const double* Qg = ps_q_slice(a.Q, a.q_mode, draw, k, &qf);
  for (int idx = tid; idx < m * nc; idx += NT) {
    const int i = idx / nc, c = idx - i * nc;
    double v;
    if (c < m) {
      v = Tg[i * m + c];
    } else {
      const int j = c - m;
      const double qjj = qf ? Qg[j * k + j] : Qg[j];
      v = (qjj > 0.0) ? Rg[i * k + j] : 0.0;
    }
    A[i * la + c] = v;
  }
  double* Ui = a.U + (size_t)draw * ks_mat(m);
  double* UTi = a.UT + (size_t)draw * ks_mat(m);
  double* URi = a.UR + (size_t)draw * ks_mat(m);
  for (size_t idx = tid; idx < ks_mat(m); idx += NT) {
    Ui[idx] = 0.0;
    UTi[idx] = 0.0;
    URi[idx] = 0.0;
  }
  int r = 0;
  double n0 = 0.0;
  for (int j = 0; j < m; ++j) {
    __syncthreads();
    if (tid < nc) {
      double s = 0.0;
      for (int i = 0; i < m; ++i) s = fma(A[i * la + tid], A[i * la + tid], s);
      cn[tid] = s;
    }
    __syncthreads();
    if (tid < 64) {  // largest remaining column (the first of equals)
      double bv = -1.0;
      int bi = 0;
      for (int c = lane; c < nc; c += 64) {
        const double v = cn[c];
        if (v > bv) { bv = v; bi = c; }
      }
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
      }
      if (lane == 0) { pvs[0] = bv; pvs[1] = (double)bi; }
    }
    __syncthreads();
    const double nr = sqrt(pvs[0]);
    const int piv = (int)pvs[1];
    if (j == 0) n0 = nr;
    if (!(nr > a.rank_tol * n0) || !(nr > 0.0)) break;  // (uniform: every thread reads the same two values)
    if (tid < m) qv[tid] = A[tid * la + piv] / nr;
    __syncthreads();
    if (tid < j) {  // second orthogonalisation against the basis so far
      double s = 0.0;
      for (int i = 0; i < m; ++i) s = fma(Uq[i * lu + tid], qv[i], s);
      hv[tid] = s;
    }
    __syncthreads();
    double qi = 0.0;
    if (tid < m) {
      qi = qv[tid];
      for (int c = 0; c < j; ++c) qi = fma(-Uq[tid * lu + c], hv[c], qi);
    }
    __syncthreads();
    if (tid < m) qv[tid] = qi;
    __syncthreads();
    double s2 = 0.0;
    for (int i = 0; i < m; ++i) s2 = fma(qv[i], qv[i], s2);
    const double inv = 1.0 / sqrt(s2);
    if (tid < m) Uq[tid * lu + j] = qi * inv;
    __syncthreads();
    if (tid < nc) {  // project the new direction out of every column
      double g = 0.0;
      for (int i = 0; i < m; ++i) g = fma(Uq[i * lu + j], A[i * la + tid], g);
      for (int i = 0; i < m; ++i) A[i * la + tid] = fma(-Uq[i * lu + j], g, A[i * la + tid]);
    }
    r = j + 1;
  }
  __syncthreads();
  const int ld = ks_ld(m);
  for (int idx = tid; idx < m * r; idx += NT) {
    const int i = idx / r, c = idx - i * r;
    Ui[i * ld + c] = Uq[i * lu + c];
  }
  for (int idx = tid; idx < r * m; idx += NT) {
    const int c = idx / m, j = idx - c * m;
    double s = 0.0;
    for (int i = 0; i < m; ++i) s = fma(Uq[i * lu + c], Tg[i * m + j], s);
    UTi[c * ld + j] = s;
  }
  for (int idx = tid; idx < r * k; idx += NT) {
    const int c = idx / k, j = idx - c * k;
    double s = 0.0;
    for (int i = 0; i < m; ++i) s = fma(Uq[i * lu + c], Rg[i * k + j], s);
    URi[c * ld + j] = s;
  }
  if (tid == 0) a.rank[draw] = r;
}

template <bool UG, bool SEG = false>
__global__ __launch_bounds__(KS_THREADS) void kalman_smoother_kernel(typename std::conditional<SEG, KsSegArgs, KsArgs>::type a) {
  constexpr int NT = KS_THREADS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63, draw = blockIdx.x, m = a.m, k = a.k, mm = m * m, n = a.T_len;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (draw >= a.batch) return;
  const size_t nv = (size_t)n * m, ncv = a.full_cov ? nv * m : nv, ne = (size_t)n * k;
  double* as_o = a.a_s ? a.a_s + (size_t)draw * nv : nullptr;
  double* ps_o = a.p_s ? a.p_s + (size_t)draw * ncv : nullptr;
  double* es_o = a.e_s ? a.e_s + (size_t)draw * ne : nullptr;
  if (a.status[draw] != 0) {  // failed solve or filter: EVERY requested output of the draw is NaN
    if (as_o) ps_fill_nan(as_o, nv, tid, NT);
    if (ps_o) ps_fill_nan(ps_o, ncv, tid, NT);
    if (es_o) ps_fill_nan(es_o, ne, tid, NT);
    return;
  }
  const int ld = ks_ld(m), mp = ks_mp(m), mt = mp / 16, m4 = ps_r4(m);
  const size_t MAT = ks_mat(m);
  // the problem whose basis, rank and Q the step uses: the draw, or (draw, segment) -- the last segment first
  int seg = 0, seg_first = 0;
  size_t prob = (size_t)draw;
  if constexpr (SEG) {
    seg = a.n_seg - 1;
    seg_first = ks_seg_start(a, seg);
    prob = (size_t)draw * a.n_seg + seg;
  }
  typename std::conditional<SEG, int, const int>::type r = a.rank[prob], rt = (r + 15) / 16, r4 = ps_r4(r);
  const bool cov = ps_o != nullptr;
  ks_lds* V = (ks_lds*)smem;
  ks_lds* Pf = V + MAT;
  ks_lds* Pp = Pf + MAT;
  ks_lds* W = Pp + MAT;
  ks_lds* pl = W + MAT;
  typedef typename std::conditional<UG, const ks_glb*, const ks_lds*>::type UPtr;
  UPtr U, UT, UR;
  ks_lds *Ul = nullptr, *UTl = nullptr, *URl = nullptr;
  if constexpr (UG) {
    U = (const ks_glb*)(a.U + prob * MAT);
    UT = (const ks_glb*)(a.UT + prob * MAT);
    UR = (const ks_glb*)(a.UR + prob * MAT);
  } else {
    Ul = pl; pl += MAT;
    UTl = pl; pl += MAT;
    URl = pl; pl += MAT;
    for (size_t idx = tid; idx < MAT; idx += NT) {
      Ul[idx] = a.U[prob * MAT + idx];
      UTl[idx] = a.UT[prob * MAT + idx];
      URl[idx] = a.UR[prob * MAT + idx];
    }
    U = Ul;
    UT = UTl;
    UR = URl;
  }
  ks_lds* as = pl; pl += 64;    // smoothed state of step t + 1
  ks_lds* dl = pl; pl += 64;    // as[t+1] - a_pred[t+1]
  ks_lds* zv = pl; pl += 64;    // z = U' dl, then M^-1 z  (w = U z is never formed: T' w = (U'T)' z, R' w = (U'R)' z)
  ks_lds* tw = pl; pl += 64;    // T' w
  ks_lds* rq = pl; pl += 64;    // R' w
  ks_lds* invd = pl; pl += 64;  // 1 / pivot
  ks_lds* apv = pl; pl += 64;   // a_pred[t+1]
  ks_lds* afv = pl; pl += 64;   // a_filt[t]
  ks_lds* qd = pl; pl += 64;    // diagonal Q
  bool qf;
  const double* Qg = ps_q_slice(a.Q, a.q_mode, prob, k, &qf);
  const double* apg = a.a_pred + (size_t)draw * nv;
  const double* afg = a.a_filt + (size_t)draw * nv;
  const double* ppg = a.p_pred + (size_t)draw * nv * m;
  const double* pfg = a.p_filt + (size_t)draw * nv * m;

  for (size_t idx = tid; idx < 4 * MAT; idx += NT) V[idx] = 0.0;  // (the padding of the four working images stays zero)
  if (es_o && tid < k) es_o[tid] = NAN;  // eps[0]
  if (tid < k) qd[tid] = qf ? Qg[tid * k + tid] : Qg[tid];
  __syncthreads();
  {  // t = n - 1: smoothed = filtered; the matrices and vectors of step n - 2
    const size_t ol = (size_t)(n - 1) * m;
    for (int idx = tid; idx < mm; idx += NT) {
      const int i = idx / m, j = idx - i * m;
      const double v = pfg[ol * m + idx];
      V[i * ld + j] = v;
      if (ps_o) {
        if (a.full_cov) ps_o[ol * m + idx] = v;
        else if (i == j) ps_o[ol + i] = v;
      }
      if (n >= 2) {
        Pp[i * ld + j] = ppg[ol * m + idx];
        Pf[i * ld + j] = pfg[(ol - m) * m + idx];
      }
    }
    if (tid < m) {
      const double v = afg[ol + tid];
      as[tid] = v;
      if (as_o) as_o[ol + tid] = v;
      if (n >= 2) {
        apv[tid] = apg[ol + tid];
        afv[tid] = afg[ol - m + tid];
      }
    }
  }
  for (int t = n - 2; t >= 0; --t) {
    const size_t ot = (size_t)t * m;
    // the matrices and vectors of step t - 1, in flight while this step computes (no other global load in the step when U
    // lives in LDS: the first use of a later load would wait for these too)
    double pfr[KS_PF] = {}, ppr[KS_PF] = {}, apr = 0.0, afr = 0.0;
    if (t > 0) {
#pragma unroll
      for (int q = 0; q < KS_PF; ++q) {
        const int idx = tid + q * NT;
        if (idx < mm) {
          pfr[q] = pfg[(ot - m) * m + idx];
          ppr[q] = ppg[ot * m + idx];
        }
      }
      if (tid < m) {
        apr = apg[ot + tid];
        afr = afg[ot - m + tid];
      }
    }
    __syncthreads();
    // (1) E = Pp U -> W;  dl;  D = V - Pp -> V
    ks_gemm<false, false>(Pp, ld, U, ld, mt, rt, m4, 0, 4, [&](int i, int j, double v) { W[i * ld + j] = v; });
    if (tid < m) dl[tid] = as[tid] - apv[tid];
    if (cov)
      for (int idx = tid; idx < mm; idx += NT) {
        const int i = idx / m, j = idx - i * m;
        V[i * ld + j] -= Pp[i * ld + j];
      }
    __syncthreads();
    // (2) M = U' E -> Pp;  z = U' dl
    ks_gemm<true, false>(U, ld, W, ld, rt, rt, m4, 0, 4, [&](int i, int j, double v) { Pp[i * ld + j] = v; });
    if (tid < r) {
      double s = 0.0;
#pragma unroll 4
      for (int i = 0; i < m; ++i) s = fma(U[i * ld + tid], dl[i], s);
      W[tid * ld + mp] = s;  // (column mp of the image: outside every product's tiles)
    }
    __syncthreads();
    // (3) M <- sym(M);  C = (U'T) P_filt -> W
    for (int i = wave; i < r; i += 4)
      for (int j = lane; j < i; j += 64) {
        const double s = 0.5 * (Pp[i * ld + j] + Pp[j * ld + i]);
        Pp[i * ld + j] = s;
        Pp[j * ld + i] = s;
      }
    if (cov) ks_gemm<false, false>(UT, ld, Pf, ld, rt, mt, m4, 0, 4, [&](int i, int j, double v) { W[i * ld + j] = v; });
    // (4) M [X | z] = [C | z] by the whole workgroup: Gauss-Jordan elimination of the positive definite system without pivoting
    // (pivot k = the square of the Cholesky factor's diagonal entry k, so "not positive definite" is the same verdict); one
    // barrier per pivot, eight rows per wavefront in flight at a time.  [First version: Cholesky and triangular solves on one
    // wavefront each -- serial loops at LDS latency: 71 us per step at m = 40 with covariances against 55 us for this form;
    // docs/design/smoother.md.]
    const int nrhs = cov ? m : 0;
    for (int kk = 0; kk < r; ++kk) {
      __syncthreads();
      const double dk = Pp[kk * ld + kk];
      if (!(dk > 0.0)) {  // (uniform) this step and every earlier one are NaN, the later ones stay
        if (as_o) ps_fill_nan(as_o, ot + m, tid, NT);
        if (ps_o) ps_fill_nan(ps_o, a.full_cov ? (ot + m) * m : ot + m, tid, NT);
        if (es_o) ps_fill_nan(es_o, (size_t)(t + 2) * k, tid, NT);
        if (tid == 0) a.status[draw] |= DSGE_ST_SMOOTHER_SINGULAR;
        return;
      }
      const double inv = 1.0 / dk;
      if (tid == 0) invd[kk] = inv;
      const int nj = r - kk - 1, ncol = nj + nrhs + 1;
      for (int ii0 = wave; ii0 < r - 1; ii0 += 32)  // eight rows per wavefront at a time: their loads are in flight together
        for (int cc = lane; cc < ncol; cc += 64) {
          const bool in_m = cc < nj;
          ks_lds* B = in_m ? Pp : W;
          const int off = in_m ? kk + 1 + cc : (cc - nj < nrhs ? cc - nj : mp);
          const double pk = B[kk * ld + off];
          double fa[8], v[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int ii = ii0 + 4 * q, i = ii < kk ? ii : ii + 1;
            if (ii < r - 1) {
              fa[q] = Pp[i * ld + kk];
              v[q] = B[i * ld + off];
            }
          }
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int ii = ii0 + 4 * q, i = ii < kk ? ii : ii + 1;
            if (ii < r - 1) B[i * ld + off] = fma(-fa[q] * inv, pk, v[q]);
          }
        }
    }
    __syncthreads();
    for (int i = wave; i < r; i += 4) {
      const double inv = invd[i];
      for (int c = lane; c < nrhs; c += 64) W[i * ld + c] *= inv;
      if (lane == 0) zv[i] = W[i * ld + mp] * inv;
    }
    __syncthreads();
    // (5) T' w = (U'T)' z, R' w = (U'R)' z;  G' = U X -> Pp
    if (tid < m) {
      double s = 0.0;
#pragma unroll 4
      for (int c = 0; c < r; ++c) s = fma(UT[c * ld + tid], zv[c], s);
      tw[tid] = s;
    } else if (tid >= 64 && tid < 64 + k) {
      const int j = tid - 64;
      double s = 0.0;
#pragma unroll 4
      for (int c = 0; c < r; ++c) s = fma(UR[c * ld + j], zv[c], s);
      rq[j] = s;
    }
    if (cov) ks_gemm<false, false>(U, ld, W, ld, mt, mt, r4, 0, 4, [&](int i, int j, double v) { Pp[i * ld + j] = v; });
    __syncthreads();
    // (6) as[t] = a_filt[t] + P_filt[t] (T' w);  eps[t+1] = Q (R' w);  F = D G' -> W
    if (tid < m) {
      double s = afv[tid];
#pragma unroll 4
      for (int j = 0; j < m; ++j) s = fma(Pf[tid * ld + j], tw[j], s);
      as[tid] = s;
      if (as_o) as_o[ot + tid] = s;
    } else if (es_o && tid >= 64 && tid < 64 + k) {
      const int j = tid - 64;
      double s;
      if (qf) {
        s = 0.0;
        for (int c = 0; c < k; ++c) s = fma(Qg[j * k + c], rq[c], s);
      } else {
        s = qd[j] * rq[j];
      }
      es_o[(size_t)(t + 1) * k + j] = s;
    }
    if (cov) {
      ks_gemm<false, false>((const ks_lds*)V, ld, (const ks_lds*)Pp, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) { W[i * ld + j] = v; });
      __syncthreads();
      // (7) S = G F -> V
      ks_gemm<true, false>(Pp, ld, W, ld, mt, mt, m4, 0, 4, [&](int i, int j, double v) { V[i * ld + j] = v; });
      __syncthreads();
      // (8) V[t] = P_filt[t] + sym(S), written out
      for (int idx = tid; idx < mm; idx += NT) {
        const int i = idx / m, j = idx - i * m;
        if (i <= j) {
          const double s = 0.5 * (V[i * ld + j] + V[j * ld + i]);
          const double vij = Pf[i * ld + j] + s, vji = Pf[j * ld + i] + s;
          V[i * ld + j] = vij;
          V[j * ld + i] = vji;
          if (a.full_cov) {
            ps_o[ot * m + idx] = vij;
            ps_o[ot * m + j * m + i] = vji;
          } else if (i == j) {
            ps_o[ot + i] = vij;
          }
        }
      }
    }
    __syncthreads();
    // (9) the matrices and vectors of step t - 1
    if (t > 0) {
#pragma unroll
      for (int q = 0; q < KS_PF; ++q) {
        const int idx = tid + q * NT;
        if (idx < mm) {
          const int i = idx / m, j = idx - i * m;
          Pf[i * ld + j] = pfr[q];
          Pp[i * ld + j] = ppr[q];
        }
      }
      if (tid < m) {
        apv[tid] = apr;
        afv[tid] = afr;
      }
    }
    if constexpr (SEG) {
      if (t + 1 == seg_first) {  // (uniform) period t belongs to the segment before: its basis, rank and Q from here on.  Nobody
        --seg;                   // reads the old ones any more, and the barrier that opens the next step publishes the new ones
        seg_first = ks_seg_start(a, seg);
        prob = (size_t)draw * a.n_seg + seg;
        r = a.rank[prob];
        rt = (r + 15) / 16;
        r4 = ps_r4(r);
        Qg = ps_q_slice(a.Q, a.q_mode, prob, k, &qf);
        if (tid < k) qd[tid] = qf ? Qg[tid * k + tid] : Qg[tid];
        if constexpr (UG) {
          U = (const ks_glb*)(a.U + prob * MAT);
          UT = (const ks_glb*)(a.UT + prob * MAT);
          UR = (const ks_glb*)(a.UR + prob * MAT);
        } else {
          for (size_t idx = tid; idx < MAT; idx += NT) {
            Ul[idx] = a.U[prob * MAT + idx];
            UTl[idx] = a.UT[prob * MAT + idx];
            URl[idx] = a.UR[prob * MAT + idx];
          }
        }
      }
    }
  }
}

}  // namespace dsge
