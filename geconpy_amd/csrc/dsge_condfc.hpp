// CONDITIONAL FORECAST per draw (hard conditions, Waggoner & Zha 1999): paths x_t = T x_{t-1} + R e_t, t = 0 .. n_steps-1, from a
// known x_{-1} = x0 that are forced through  d[j_c] + Z[j_c, :] x[t_c] = v_c,  c < n_cond, by the correction of the free shocks
// F in periods 0 .. t_max of minimum Q_FF^-1 norm.  With Psi_l = Z T^l R and W[c, (s, f)] = Psi_{t_c - s}[j_c, f] (s <= t_c):
//     G = W (I (x) Q_FF) W' = L L',   lambda = G^-1 r,   Delta_s = Q_FF sum_{c: t_c >= s} Psi_{t_c - s}[j_c, F]' lambda_c,   e = e+ + Delta
// W is block-Toeplitz and never exists as an array.
//
// condfc_setup_kernel, one workgroup per draw (everything that does not depend on the path): T in one zero-padded LDS image, the
// rows V_l = Z T^l (p <= 16: the 16 columns of ONE matrix-core tile, stored path-major like the x image of the dynamics kernels)
// advanced by one ks_gemm per lag, V_{l+1}' = T' V_l'; Psi_l = V_l R and PsiQ_l = Psi_l[:, F] Q_FF on the VALU, written to library
// scratch as they appear (their number grows with t_max, so they do not live in the LDS); G from the Toeplitz sums; its Cholesky
// factor in LDS with the pivot test  pivot <= rank_tol max_c G[c, c]  ->  DSGE_ST_COND_SINGULAR; L (packed) to scratch.
//
// condfc_paths_kernel, one workgroup of 256 threads per (draw, 16 paths): the [T | R] image, the path-major double-buffered
// [x ; e] image and the row stride of dynamics_propagate_kernel (dsge_dynamics.hpp).  Pass 1 propagates the baseline e+ to t_max,
// writes nothing to memory and collects r_c = v_c - d[j_c] - Z[j_c] x+[t_c] of the 16 paths; two triangular solves, one thread
// per path; Delta in the Psi form above (n_cond (t_max + 1) |F| products per path against (t_max + 1) m^2 of the costate
// recursion, no third propagation, and PsiQ exists already because G needs it); pass 2 propagates e+ + Delta and writes each
// slab of x, e and d + Z x once, with one barrier per step.  No atomics: two calls give the same bits.  A shock that is not free
// is never added to, so it comes back with the bits it came with.
// Shared pieces (dsge_postsolve.hpp) this file calls, and the lines it keeps: docs/design/dynamics.md, "the shared pieces".
#pragma once
#include "dsge_postsolve.hpp"

namespace dsge {

constexpr int CF_THREADS = 256, CF_COLS = 16, CF_MAX_COND = 64;
constexpr int CF_ST_SINGULAR = 512;  // DSGE_ST_COND_SINGULAR
constexpr int CF_EPF = 6;  // CF_EPF * CF_THREADS >= CF_COLS * DSGE_MAX_N_BIG: the shocks of one step in flight


__host__ __device__ inline size_t cf_tri(int n) { return (size_t)n * (n + 1) / 2; }
// the setup kernel: T, two V images, R, the masked Q, two Psi_l, G [n_cond][n_cond + 1], the diagonal of L
__host__ __device__ inline size_t cf_setup_lds_doubles(int m, int k, int n_cond) {
  return ks_mat(m) + 2 * (size_t)CF_COLS * ks_ld(m) + (size_t)m * k + (size_t)k * k + 2 * (size_t)CF_COLS * k +
         (size_t)n_cond * (n_cond + 1) + n_cond;
}
// the paths kernel: [T | R], two [x ; e] images, Z, d, r / lambda [n_cond][17], and ONE region for L (packed, during the solves) and
// Delta [(t_max + 1) |F|][16] (after them)
__host__ __device__ inline size_t cf_paths_lds_doubles(int m, int k, int p, int n_cond, int lags, int n_free) {
  const size_t tri = cf_tri(n_cond), del = (size_t)lags * n_free * CF_COLS;
  return (size_t)(ks_mp(m) + 2 * CF_COLS) * ps_ld(m, k) + (size_t)p * m + CF_COLS + (size_t)n_cond * (CF_COLS + 1) +
         (tri > del ? tri : del);
}

struct CondFcArgs {
  const double* T;         // [batch][m][m]
  const double* R;         // [batch][m][k]
  const double* Q;         // layout q_mode
  const double* Z;         // [batch | 1][p][m]
  const double* d;         // [batch | 1][p] or nullptr
  const double* x0;        // element (draw, path, i) at draw x0_draw + path x0_path + i
  const double* eps;       // [batch | 1][n_paths][n_shock_steps][k] or nullptr (zero)
  const double* cond_val;  // element (draw, path, c) at draw cv_draw + path cv_path + c
  int32_t* status;         // [batch] in/out or nullptr
  double* x_out;           // [batch][n_paths][n_steps][m] or nullptr
  double* eps_out;         // [batch][n_paths][n_steps][k] or nullptr
  double* obs_out;         // [batch][n_paths][n_steps][p] or nullptr
  double* chol;            // scratch [batch][n_cond (n_cond + 1) / 2]: L, row-packed
  double* psi;             // scratch [batch][t_max + 1][p][k]: Psi_l
  double* psiq;            // scratch [batch][t_max + 1][p][k]: Psi_l[:, F] Q_FF (zero outside F)
  int32_t* flag;           // scratch [batch]: non-zero = the draw gets NaN
  long long* dbg;          // debug (dsge_debug_condfc_phases): int64[8], shader-clock cycles of wavefront 0 of workgroup 0
  long long x0_draw, x0_path, eps_draw, cv_draw, cv_path;
  double rank_tol;
  int batch, m, k, p, n_paths, n_steps, n_shock_steps, n_cond, t_max, n_free, q_mode, z_batched, d_batched, groups;
  int cond_t[CF_MAX_COND];
  unsigned char cond_j[CF_MAX_COND];
  unsigned char free_idx[DSGE_MAX_N_BIG];  // the free shocks, ascending
  signed char free_pos[DSGE_MAX_N_BIG];    // position of shock j in free_idx, -1: not free
};

__global__ __launch_bounds__(CF_THREADS) void condfc_setup_kernel(CondFcArgs a) {
  constexpr int NT = CF_THREADS, NC = CF_COLS;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, draw = blockIdx.x, m = a.m, k = a.k, p = a.p, n = a.n_cond, lags = a.t_max + 1;
  if (draw >= a.batch) return;
  if (a.status && a.status[draw] != 0) {  // failed solve: the paths kernel writes NaN
    if (tid == 0) a.flag[draw] = 1;
    return;
  }
  const bool prof = a.dbg != nullptr && blockIdx.x == 0 && tid < 64;
  const long long p_begin = prof ? clock64() : 0;
  const int ld = ks_ld(m), mt = ks_mp(m) / 16, m4 = ps_r4(m), ldg = n + 1, pk = p * k;
  ks_lds* Tm = (ks_lds*)smem;             // [mp][ld]
  ks_lds* Vc = Tm + ks_mat(m);            // [NC][ld]: row o of V_l in Vc[o ld + 0 .. m-1]
  ks_lds* Vn = Vc + NC * ld;
  ks_lds* Rm = Vn + NC * ld;              // [m][k]
  ks_lds* Qm = Rm + m * k;                // [k][k]: Q with the rows and columns of the shocks that are not free zeroed
  ks_lds* ps = Qm + k * k;                // [2][NC k]: Psi_l by the parity of l
  ks_lds* G = ps + 2 * NC * k;            // [n][ldg]
  ks_lds* dg = G + n * ldg;               // [n]: the diagonal of L
  for (size_t idx = tid; idx < cf_setup_lds_doubles(m, k, n); idx += NT) Tm[idx] = 0.0;
  __syncthreads();
  const double* Tg = a.T + (size_t)draw * m * m;
  const double* Rg = a.R + (size_t)draw * m * k;
  const double* Zg = a.Z + (a.z_batched ? (size_t)draw * p * m : 0);
  for (int idx = tid; idx < m * m; idx += NT) {
    const int i = idx / m, j = idx - i * m;
    Tm[i * ld + j] = Tg[idx];
  }
  for (int idx = tid; idx < m * k; idx += NT) Rm[idx] = Rg[idx];
  for (int idx = tid; idx < p * m; idx += NT) {
    const int o = idx / m, i = idx - o * m;
    Vc[o * ld + i] = Zg[idx];
  }
  {
    const bool qb = a.q_mode == DSGE_Q_DIAG_BATCHED || a.q_mode == DSGE_Q_FULL_BATCHED;
    const bool qf = a.q_mode == DSGE_Q_FULL_SHARED || a.q_mode == DSGE_Q_FULL_BATCHED;
    const double* Qg = a.Q + (qb ? (size_t)draw * (qf ? k * k : k) : 0);
    for (int idx = tid; idx < k * k; idx += NT) {
      const int e = idx / k, f = idx - e * k;
      if (a.free_pos[e] >= 0 && a.free_pos[f] >= 0) Qm[idx] = qf ? Qg[idx] : (e == f ? Qg[e] : 0.0);
    }
  }
  __syncthreads();
  double* psg = a.psi + (size_t)draw * lags * pk;
  double* pqg = a.psiq + (size_t)draw * lags * pk;
  for (int l = 0; l < lags; ++l) {  // Psi_l = V_l R while V_{l+1}' = T' V_l' multiplies; one barrier per lag
    ks_lds* pb = ps + (l & 1) * NC * k;
    for (int idx = tid; idx < pk; idx += NT) {
      const int o = idx / k, f = idx - o * k;
      double s = 0.0;
      for (int i = 0; i < m; ++i) s = fma(Vc[o * ld + i], Rm[i * k + f], s);
      pb[idx] = s;
      psg[(size_t)l * pk + idx] = s;
    }
    if (l + 1 < lags)
      ks_gemm<true, true>((const ks_lds*)Tm, ld, (const ks_lds*)Vc, ld, mt, 1, m4, 0, 4, [&](int i, int j, double v) {
        if (i < m4) Vn[j * ld + i] = v;
      });
    __syncthreads();
    for (int idx = tid; idx < pk; idx += NT) {
      const int o = idx / k, f = idx - o * k;
      double s = 0.0;
      for (int e = 0; e < k; ++e) s = fma(pb[o * k + e], Qm[e * k + f], s);
      pqg[(size_t)l * pk + idx] = s;
    }
    ks_lds* sw = Vc;
    Vc = Vn;
    Vn = sw;
  }
  __syncthreads();  // (Psi and PsiQ of this draw, written by this workgroup, are read back below)
  const long long p_psi = prof ? clock64() : 0;
  // G[c, c'] = sum_{s <= min(t_c, t_c')} PsiQ_{t_c - s}[j_c, :] . Psi_{t_c' - s}[j_c', :], the lower triangle, mirrored
  for (int idx = tid; idx < n * n; idx += NT) {
    const int c = idx / n, c2 = idx - c * n;
    if (c2 > c) continue;
    const int tc = a.cond_t[c], tc2 = a.cond_t[c2], jc = a.cond_j[c], jc2 = a.cond_j[c2];  // (tc2 <= tc: the pairs ascend)
    double s = 0.0;
    for (int q = 0; q <= tc2; ++q) {
      const double* u = pqg + ((size_t)(tc - q) * p + jc) * k;
      const double* v = psg + ((size_t)(tc2 - q) * p + jc2) * k;
      for (int f = 0; f < k; ++f) s = fma(u[f], v[f], s);
    }
    G[c * ldg + c2] = s;
    G[c2 * ldg + c] = s;
  }
  __syncthreads();
  const long long p_g = prof ? clock64() : 0;
  double gmax = 0.0;
  for (int c = 0; c < n; ++c) gmax = fmax(gmax, G[c * ldg + c]);
  bool nan_diag = false;
  for (int c = 0; c < n; ++c) nan_diag |= !(G[c * ldg + c] == G[c * ldg + c]);
  const double thr = (a.rank_tol > 0.0 ? a.rank_tol : 1e-10) * gmax;
  bool singular = nan_diag;
  for (int j = 0; j < n && !singular; ++j) {  // right-looking Cholesky, the lower triangle; every thread sees the same pivot
    const double piv = G[j * ldg + j];
    if (!(piv > thr)) {
      singular = true;
      break;
    }
    const double r = sqrt(piv);
    if (tid == 0) dg[j] = r;
    for (int i = j + 1 + tid; i < n; i += NT) G[i * ldg + j] /= r;
    __syncthreads();
    const int w = n - j - 1;
    for (int idx = tid; idx < w * w; idx += NT) {
      const int i = j + 1 + idx / w, c = j + 1 + idx % w;
      if (c <= i) G[i * ldg + c] = fma(-G[i * ldg + j], G[c * ldg + j], G[i * ldg + c]);
    }
    __syncthreads();
  }
  if (singular) {
    if (tid == 0) {
      a.flag[draw] = 1;
      if (a.status) a.status[draw] |= CF_ST_SINGULAR;
    }
  } else {
    if (tid == 0) a.flag[draw] = 0;
    double* Lg = a.chol + (size_t)draw * cf_tri(n);
    for (int idx = tid; idx < n * n; idx += NT) {
      const int c = idx / n, c2 = idx - c * n;
      if (c2 <= c) Lg[cf_tri(c) + c2] = c2 == c ? dg[c] : G[c * ldg + c2];
    }
  }
  if (prof && tid == 0) {
    a.dbg[0] = p_psi - p_begin;
    a.dbg[1] = p_g - p_psi;
    a.dbg[2] = clock64() - p_g;
  }
}

__global__ __launch_bounds__(CF_THREADS) void condfc_paths_kernel(CondFcArgs a) {
  constexpr int NT = CF_THREADS, NC = CF_COLS, LR = CF_COLS + 1;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, m = a.m, k = a.k, p = a.p, n = a.n_cond, n_steps = a.n_steps;
  const int draw = blockIdx.x / a.groups, g = blockIdx.x - draw * a.groups;
  if (draw >= a.batch) return;
  const int s0 = g * NC, nc = a.n_paths - s0 < NC ? a.n_paths - s0 : NC;
  const size_t path0 = (size_t)draw * a.n_paths + s0;
  double* xo = a.x_out ? a.x_out + path0 * n_steps * m : nullptr;
  double* eo = a.eps_out ? a.eps_out + path0 * n_steps * k : nullptr;
  double* oo = a.obs_out ? a.obs_out + path0 * n_steps * p : nullptr;
  if ((a.status && a.status[draw] != 0) || (n > 0 && a.flag[draw] != 0)) {  // failed or singular: EVERY output of the draw is NaN
    if (xo) for (size_t i = tid; i < (size_t)nc * n_steps * m; i += NT) xo[i] = NAN;
    if (eo) for (size_t i = tid; i < (size_t)nc * n_steps * k; i += NT) eo[i] = NAN;
    if (oo) for (size_t i = tid; i < (size_t)nc * n_steps * p; i += NT) oo[i] = NAN;
    return;
  }
  const bool prof = a.dbg != nullptr && blockIdx.x == 0 && tid < 64;
  const long long p_begin = prof ? clock64() : 0;
  const int m4 = ps_r4(m), k4 = ps_r4(k), mp = ks_mp(m), mt = mp / 16, ld = ps_ld(m, k), lags = a.t_max + 1, nF = a.n_free;
  ks_lds* TR = (ks_lds*)smem;       // [mp][ld]: T in columns 0 .. m-1, R in columns m4 .. m4+k-1
  ks_lds* cur = TR + mp * ld;       // [NC][ld]: x_{t-1} of path j in cur[j ld + 0 .. m-1], e_t in cur[j ld + m4 .. m4+k-1]
  ks_lds* nxt = cur + NC * ld;
  ks_lds* Zm = nxt + NC * ld;       // [p][m]
  ks_lds* dv = Zm + p * m;          // [NC]
  ks_lds* rl = dv + NC;             // [n][LR]: r, then lambda, of path j in rl[c LR + j]
  ks_lds* Lp = rl + n * LR;         // L, row-packed, during the solves;
  ks_lds* Dl = Lp;                  // afterwards Delta: shock free_idx[fi] of period s, path j in Dl[(s nF + fi) NC + j]
  for (size_t idx = tid; idx < cf_paths_lds_doubles(m, k, p, n, n > 0 ? lags : 0, nF); idx += NT) TR[idx] = 0.0;
  __syncthreads();
  const double* Tg = a.T + (size_t)draw * m * m;
  const double* Rg = a.R + (size_t)draw * m * k;
  for (int idx = tid; idx < m * m; idx += NT) {
    const int i = idx / m, j = idx - i * m;
    TR[i * ld + j] = Tg[idx];
  }
  for (int idx = tid; idx < m * k; idx += NT) {
    const int i = idx / k, c = idx - i * k;
    TR[i * ld + m4 + c] = Rg[idx];
  }
  {
    const double* Zg = a.Z + (a.z_batched ? (size_t)draw * p * m : 0);
    for (int idx = tid; idx < p * m; idx += NT) Zm[idx] = Zg[idx];
    if (tid < p) dv[tid] = a.d ? ps_obs_slice(a.d, a.d_batched, draw, p)[tid] : 0.0;
  }
  const double* xg = a.x0 + (size_t)draw * a.x0_draw + (size_t)s0 * a.x0_path;
  auto load_x0 = [&]() {
    for (int idx = tid; idx < nc * m; idx += NT) {
      const int j = idx / m, i = idx - j * m;
      cur[j * ld + i] = xg[(size_t)j * a.x0_path + i];
    }
  };
  const int nsh = a.eps ? a.n_shock_steps : 0;
  const size_t per_path = (size_t)a.n_shock_steps * k;
  const double* eg = a.eps ? a.eps + (size_t)draw * a.eps_draw + (size_t)s0 * per_path : nullptr;
  auto base = [&](int idx, int t) -> double {  // entry idx = j k + c of the baseline e+_t
    return t < nsh ? eg[(size_t)(idx / k) * per_path + (size_t)t * k + idx % k] : 0.0;
  };
  long long p_pass1 = 0, p_solve = 0, p_delta = 0;
  if (n > 0) {
    // ---- pass 1: the baseline to t_max, nothing written; r_c of the 16 paths ----
    load_x0();
    if (nsh > 0)
      for (int idx = tid; idx < nc * k; idx += NT) cur[(idx / k) * ld + m4 + idx % k] = base(idx, 0);
    __syncthreads();
    const double* cv = a.cond_val + (size_t)draw * a.cv_draw + (size_t)s0 * a.cv_path;
    int c_lo = 0;
    for (int t = 0; t <= a.t_max; ++t) {
      const bool more = t + 1 < nsh;
      double ev[CF_EPF] = {};
      if (more) {
#pragma unroll
        for (int q = 0; q < CF_EPF; ++q) {
          const int idx = tid + q * NT;
          if (idx < nc * k) ev[q] = base(idx, t + 1);
        }
      }
      ks_gemm<false, true>((const ks_lds*)TR, ld, (const ks_lds*)cur, ld, mt, 1, t < nsh ? m4 + k4 : m4, 0, 4,
                           [&](int i, int j, double v) {
                             if (i < m4) nxt[j * ld + i] = v;
                           });
      if (more) {
#pragma unroll
        for (int q = 0; q < CF_EPF; ++q) {
          const int idx = tid + q * NT;
          if (idx < nc * k) nxt[(idx / k) * ld + m4 + idx % k] = ev[q];
        }
      }
      __syncthreads();
      int c_hi = c_lo;
      while (c_hi < n && a.cond_t[c_hi] == t) ++c_hi;
      for (int idx = tid; idx < (c_hi - c_lo) * NC; idx += NT) {
        const int c = c_lo + idx / NC, j = idx % NC;
        if (j < nc) {
          const int o = a.cond_j[c];
          double s = 0.0;
          for (int i = 0; i < m; ++i) s = fma(Zm[o * m + i], nxt[j * ld + i], s);
          rl[c * LR + j] = cv[(size_t)j * a.cv_path + c] - dv[o] - s;
        }
      }
      c_lo = c_hi;
      ps_swap(cur, nxt);
    }
    const double* Lg = a.chol + (size_t)draw * cf_tri(n);
    for (int idx = tid; idx < (int)cf_tri(n); idx += NT) Lp[idx] = Lg[idx];
    __syncthreads();
    p_pass1 = prof ? clock64() : 0;
    // ---- L y = r, L' lambda = y: one thread per path, in place ----
    if (tid < nc) {
      for (int c = 0; c < n; ++c) {
        const ks_lds* row = Lp + cf_tri(c);
        double s = rl[c * LR + tid];
        for (int c2 = 0; c2 < c; ++c2) s = fma(-row[c2], rl[c2 * LR + tid], s);
        rl[c * LR + tid] = s / row[c];
      }
      for (int c = n - 1; c >= 0; --c) {
        double s = rl[c * LR + tid];
        for (int c2 = c + 1; c2 < n; ++c2) s = fma(-Lp[cf_tri(c2) + c], rl[c2 * LR + tid], s);
        rl[c * LR + tid] = s / Lp[cf_tri(c) + c];
      }
    }
    __syncthreads();
    p_solve = prof ? clock64() : 0;
    // ---- Delta_s[f] = sum_{c: t_c >= s} PsiQ_{t_c - s}[j_c, f] lambda_c, ascending c (over the region L was in) ----
    const double* pqg = a.psiq + (size_t)draw * lags * p * k;
    for (int idx = tid; idx < lags * nF * NC; idx += NT) {
      const int j = idx % NC, sf = idx / NC, s_ = sf / nF, f = a.free_idx[sf - s_ * nF];
      double s = 0.0;
      if (j < nc)
        for (int c = 0; c < n; ++c) {
          const int l = a.cond_t[c] - s_;
          if (l >= 0) s = fma(pqg[((size_t)l * p + a.cond_j[c]) * k + f], rl[c * LR + j], s);
        }
      Dl[idx] = s;
    }
    __syncthreads();
    p_delta = prof ? clock64() : 0;
  }
  // ---- pass 2: e = e+ + Delta, every slab written once ----
  const int n_eff = n > 0 && lags > nsh ? lags : nsh;  // periods with a shock that may be non-zero
  auto shock = [&](int idx, int t) -> double {
    const int j = idx / k, c = idx - j * k;
    double v = base(idx, t);
    if (n > 0 && t < lags && a.free_pos[c] >= 0) v += Dl[(t * nF + a.free_pos[c]) * NC + j];
    return v;
  };
  load_x0();
  for (int idx = tid; idx < nc * k; idx += NT) {
    const int j = idx / k, c = idx - j * k;
    const double v = n_eff > 0 ? shock(idx, 0) : 0.0;
    cur[j * ld + m4 + c] = v;
    if (eo) eo[(size_t)j * n_steps * k + c] = v;
  }
  __syncthreads();
  for (int t = 0; t < n_steps; ++t) {
    const bool more = t + 1 < n_eff;
    double ev[CF_EPF] = {};  // e_{t+1}, in flight while this step multiplies
    if (more) {
#pragma unroll
      for (int q = 0; q < CF_EPF; ++q) {
        const int idx = tid + q * NT;
        if (idx < nc * k) ev[q] = shock(idx, t + 1);
      }
    }
    ks_gemm<false, true>((const ks_lds*)TR, ld, (const ks_lds*)cur, ld, mt, 1, t < n_eff ? m4 + k4 : m4, 0, 4,
                         [&](int i, int j, double v) {
                           if (i < m4) nxt[j * ld + i] = v;
                         });
    if (t + 1 < n_steps) {
#pragma unroll
      for (int q = 0; q < CF_EPF; ++q) {
        const int idx = tid + q * NT;
        if (idx < nc * k) {
          const int j = idx / k, c = idx - j * k;
          if (more) nxt[j * ld + m4 + c] = ev[q];
          if (eo) eo[((size_t)j * n_steps + t + 1) * k + c] = ev[q];  // (zero past the last shock)
        }
      }
    }
    __syncthreads();
    if (xo)
      for (int idx = tid; idx < nc * m; idx += NT) {  // the slab of this step: m contiguous doubles per path
        const int j = idx / m, i = idx - j * m;
        xo[((size_t)j * n_steps + t) * m + i] = nxt[j * ld + i];
      }
    if (oo)
      for (int idx = tid; idx < nc * p; idx += NT) {
        const int j = idx / p, o = idx - j * p;
        double s = 0.0;
        for (int i = 0; i < m; ++i) s = fma(Zm[o * m + i], nxt[j * ld + i], s);
        oo[((size_t)j * n_steps + t) * p + o] = dv[o] + s;
      }
    ps_swap(cur, nxt);
  }
  if (prof && tid == 0) {
    const long long p_end = clock64();
    a.dbg[3] = n > 0 ? p_pass1 - p_begin : 0;
    a.dbg[4] = n > 0 ? p_solve - p_pass1 : 0;
    a.dbg[5] = n > 0 ? p_delta - p_solve : 0;
    a.dbg[6] = p_end - (n > 0 ? p_delta : p_begin);
    a.dbg[7] = p_end - p_begin;
  }
}

}  // namespace dsge
