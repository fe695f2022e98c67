// STOCHASTIC SIMULATION AT AN OCCASIONALLY BINDING BOUND per draw: the bound of dsge_obc.hpp with SURPRISE shocks.  A new shock
// eps_t arrives every period, agents re-plan, and the linear complementarity problem of dsge_obc.hpp is solved again every period:
//     xu   = T x_{t-1} + R eps_t                                     (the next state if no shadow shock is used)
//     q_h  = c'T^h xu - bound                       h = 0 .. H-1      (the expected gaps on that path)
//     nu   = the regime iteration on (Mz, q)                          (Mz is the draw's, the same matrix every period)
//     x_t  = xu + W nu,     W[:, j] = G^j R[:, s]                     (period 0 of the plan's path)
// Mz, Cq[h] = c'T^h (H x n) and W (n x H) are constant per draw, so the whole simulation is one launch after a per-draw setup:
//   obc_sim_setup_kernel  per draw, T and G in the LDS: wavefront 0 the chain Cq[h+1] = Cq[h] T, wavefront 1 the chain
//                         W[:, j+1] = G W[:, j], both with the running vector in a register (readlane_dyn_f64) and sums in ascending
//                         index; tables to library scratch, Cq [H][n] and W transposed [H][n].  A skipped draw writes nothing;
//   obc_sim_kernel<HM>    one wavefront per (draw, path), the four wavefronts of a workgroup on paths of ONE draw whose tables are
//                         staged once in the LDS with odd leading dimensions: Mz [H][H+1], Cq [H][n+1], W [n][H+1], T [n][n+1] and,
//                         where the host found room (obc_sim_r_in_lds), R [n][k|1] -- otherwise R is read from global memory.  The
//                         time loop runs inside the kernel: lane i forms row i of xu and of x, lane h forms q_h, lane c fetches
//                         eps_t[c]; x, xu and nu are
//                         exchanged through 64-double LDS slots of the wavefront; the regime iteration is obc_regime_iterate of
//                         dsge_obc_regime.hpp.  Rows of x, observed and the plan are written as the loop goes.  A path that fails at
//                         period t_f keeps the periods before it and gets NaN from t_f on;
//   obc_sim_status_kernel the draw's status bit from its paths' bits.
// No atomics: two calls give the same bits.
#pragma once
#include "dsge_obc_regime.hpp"

namespace dsge {

constexpr int OBC_HORIZON_SHORT = 16;  // DSGE_OBC_HORIZON_SHORT
constexpr int OBC_SIM_SETUP_THREADS = 128;
constexpr int OBC_SIM_SLOTS = 3;  // x, xu, nu: 64 doubles each per wavefront

__host__ __device__ inline int obc_sim_ldr(int k) { return k | 1; }
// Mz, Cq, W, T and the slots of the four wavefronts; R behind them
__host__ __device__ inline size_t obc_sim_lds_doubles(int H, int m, int k, bool r_lds) {
  return (size_t)H * (H + 1) + (size_t)H * (m + 1) + (size_t)m * (H + 1) + (size_t)m * (m + 1) + OBC_WAVES * OBC_SIM_SLOTS * 64 +
         (r_lds ? (size_t)m * obc_sim_ldr(k) : 0);
}
// at most 139 264 bytes without R (n = H = 64); R joins where the whole image stays within `limit` bytes
__host__ __device__ inline bool obc_sim_r_in_lds(int H, int m, int k, size_t limit) {
  return obc_sim_lds_doubles(H, m, k, true) * sizeof(double) <= limit;
}
__host__ __device__ inline size_t obc_sim_setup_lds_doubles(int m) { return (size_t)2 * m * (m + 1); }

struct ObcSimArgs {
  const double* T;       // [batch][m][m]
  const double* R;       // [batch][m][k]
  const double* G;       // [batch][m][m]
  const double* mzt;     // [batch][H][H]: Mz[h][j] at j H + h
  const double* c_row;   // [batch | 1][m]
  const double* bound;   // [batch | 1]
  const double* eps;     // [batch | 1][n_paths][n_shock_steps][k], or nullptr with n_shock_steps == 0
  const double* x0;      // [batch | 1][n_paths | 1][m] or nullptr
  const double* Z;       // [batch | 1][p][m] or nullptr
  const double* d;       // [batch | 1][p] or nullptr
  int32_t* status;       // [batch] in/out or nullptr
  const int32_t* flag;   // [batch]: non-zero = M singular
  double* cq;            // [batch][H][m]: Cq[h] = c'T^h
  double* wt;            // [batch][H][m]: W[:, j] = G^j R[:, s] at row j
  int32_t* pstat;        // [batch][n_paths]
  double* x_out;         // the caller's, or nullptr
  double* obs_out;
  double* gap_out;
  double* shadow_out;
  double* plan_out;
  int32_t* duration_out;
  int32_t* iters_out;
  double* Mz_out;
  int32_t* pstat_out;
  int32_t* fail_out;
  long long eps_draw;
  double rank_tol;
  int batch, m, k, p, n_paths, n_steps, n_shock_steps, H, shock, max_iter, c_batched, b_batched, x0_batched, x0_paths, z_batched,
      d_batched, groups, r_lds;
};

__device__ __forceinline__ bool obc_sim_skipped(const ObcSimArgs& a, int draw) {
  return (a.status && a.status[draw] != 0) || a.flag[draw] != 0;
}

// v into slot[lane], visible to the wavefront's lanes afterwards
__device__ __forceinline__ void obc_sim_put(ks_lds* slot, int lane, double v) {
  __builtin_amdgcn_wave_barrier();
  slot[lane] = v;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(OBC_SIM_SETUP_THREADS) void obc_sim_setup_kernel(ObcSimArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, H = a.H, m = a.m, k = a.k, ld = m + 1;
  const int draw = blockIdx.x;
  if (obc_sim_skipped(a, draw)) return;  // (the whole workgroup)
  ks_lds* Tm = (ks_lds*)smem;  // [m][ld]
  ks_lds* Gm = Tm + m * ld;    // [m][ld]
  ps_stage_T(Tm, ld, a.T + (size_t)draw * m * m, m, tid, OBC_SIM_SETUP_THREADS);
  ps_stage_T(Gm, ld, a.G + (size_t)draw * m * m, m, tid, OBC_SIM_SETUP_THREADS);
  __syncthreads();
  const bool on = lane < m;
  const int li = on ? lane : 0;
  if (wv == 0) {
    // Cq[0] = c,  Cq[h + 1][j] = sum_i Cq[h][i] T[i][j], ascending i
    double* out = a.cq + (size_t)draw * H * m;
    double v = on ? ps_obs_slice(a.c_row, a.c_batched, draw, m)[lane] : 0.0;
    for (int h = 0; h < H; ++h) {
      if (on) out[h * m + lane] = v;
      double acc = 0.0;
      for (int i = 0; i < m; ++i) acc = fma(readlane_dyn_f64(v, i), Tm[i * ld + li], acc);
      v = on ? acc : 0.0;
    }
  } else {
    // W[:, 0] = R[:, s],  W[i][j + 1] = sum_c G[i][c] W[c][j], ascending c
    double* out = a.wt + (size_t)draw * H * m;
    double v = on ? a.R[((size_t)draw * m + lane) * k + a.shock] : 0.0;
    for (int j = 0; j < H; ++j) {
      if (on) out[j * m + lane] = v;
      double acc = 0.0;
      for (int c = 0; c < m; ++c) acc = fma(Gm[li * ld + c], readlane_dyn_f64(v, c), acc);
      v = on ? acc : 0.0;
    }
  }
}

// sum_j a[j] b[j] in one fixed order: four interleaved partial sums (j mod 4, the tail on the first), then (s0 + s1) + (s2 + s3).
// One chain of n dependent fma would wait for the LDS once per term at the one or two wavefronts per SIMD this kernel has
__device__ __forceinline__ double obc_sim_dot(const ks_lds* a, const ks_lds* b, int n) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int j = 0;
  for (; j + 4 <= n; j += 4) {
    s0 = fma(a[j], b[j], s0);
    s1 = fma(a[j + 1], b[j + 1], s1);
    s2 = fma(a[j + 2], b[j + 2], s2);
    s3 = fma(a[j + 3], b[j + 3], s3);
  }
  for (; j < n; ++j) s0 = fma(a[j], b[j], s0);
  return (s0 + s1) + (s2 + s3);
}

// HM: 32 or 64, the rows of K a lane holds in the regime iteration
template <int HM>
__global__ __launch_bounds__(OBC_THREADS) void obc_sim_kernel(ObcSimArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, H = a.H, m = a.m, k = a.k, p = a.p, n_steps = a.n_steps;
  const int draw = blockIdx.x / a.groups, g = blockIdx.x - draw * a.groups;
  if (draw >= a.batch) return;
  const int path = g * OBC_WAVES + wv, ldh = H + 1, ldm = m + 1, ldr = obc_sim_ldr(k);
  ks_lds* Mz = (ks_lds*)smem;                                 // [H][ldh]
  ks_lds* Cq = Mz + H * ldh;                                  // [H][ldm]
  ks_lds* W = Cq + H * ldm;                                   // [m][ldh]
  ks_lds* Tm = W + m * ldh;                                   // [m][ldm]
  ks_lds* xs = Tm + m * ldm + wv * (OBC_SIM_SLOTS * 64);      // [64]: x_{t-1}, then x_t
  ks_lds* us = xs + 64;                                       // [64]: xu
  ks_lds* nub = us + 64;                                      // [64]: nu
  ks_lds* Rm = Tm + m * ldm + OBC_WAVES * OBC_SIM_SLOTS * 64;  // [m][ldr] with r_lds
  const bool skipped = obc_sim_skipped(a, draw);  // (the whole workgroup)
  const double* mg = a.mzt + (size_t)draw * H * H;
  for (int idx = tid; idx < H * H; idx += OBC_THREADS) {
    const int j = idx / H, h = idx - j * H;
    Mz[h * ldh + j] = mg[idx];
  }
  if (!skipped) {  // (a skipped draw has no tables)
    const double* cg = a.cq + (size_t)draw * H * m;
    const double* wg = a.wt + (size_t)draw * H * m;
    for (int idx = tid; idx < H * m; idx += OBC_THREADS) {
      const int h = idx / m, i = idx - h * m;
      Cq[h * ldm + i] = cg[idx];
      W[i * ldh + h] = wg[idx];
    }
    ps_stage_T(Tm, ldm, a.T + (size_t)draw * m * m, m, tid, OBC_THREADS);
    if (a.r_lds) {
      const double* rg = a.R + (size_t)draw * m * k;
      for (int idx = tid; idx < m * k; idx += OBC_THREADS) {
        const int i = idx / k, c = idx - i * k;
        Rm[i * ldr + c] = rg[idx];
      }
    }
  }
  __syncthreads();
  if (a.Mz_out && g == 0) {  // (NaN for a draw that was skipped: the unit paths' kernel has filled it)
    double* mo = a.Mz_out + (size_t)draw * H * H;
    for (int idx = tid; idx < H * H; idx += OBC_THREADS) {
      const int h = idx / H, j = idx - h * H;
      mo[idx] = Mz[h * ldh + j];
    }
  }
  if (path >= a.n_paths) return;  // (no barrier below)
  const size_t pi = (size_t)draw * a.n_paths + path, row0 = pi * n_steps;
  const bool act = lane < H, on = lane < m;
  const int li = on ? lane : 0;
  int st = skipped ? OBC_SKIPPED : 0, fail = skipped ? 0 : -1, fail_iters = 0;
  if (!skipped) {
    const double* cr = ps_obs_slice(a.c_row, a.c_batched, draw, m);
    const double bnd = a.bound[a.b_batched ? draw : 0], ci = on ? cr[lane] : 0.0;
    double mmax = 0.0;
    if (act)
      for (int c = 0; c < H; ++c) mmax = fmax(mmax, fabs(Mz[lane * ldh + c]));
    for (int off = 32; off >= 1; off >>= 1) mmax = fmax(mmax, __shfl_xor(mmax, off));
    const double thr = (a.rank_tol > 0.0 ? a.rank_tol : 1e-14) * mmax;
    const int max_iter = a.max_iter > 0 ? a.max_iter : 64, nsh = a.n_shock_steps;
    const double* eg = nsh > 0 ? a.eps + (size_t)draw * a.eps_draw + (size_t)path * nsh * k : nullptr;
    const double* rg = a.R + ((size_t)draw * m + (on ? lane : 0)) * k;
    const double* zg = p > 0 ? ps_obs_slice(a.Z, a.z_batched, draw, p * m) + (size_t)(lane < p ? lane : 0) * m : nullptr;
    const double dv = a.d && lane < p ? ps_obs_slice(a.d, a.d_batched, draw, p)[lane] : 0.0;
    double x = 0.0;
    if (a.x0 && on) x = a.x0[((size_t)(a.x0_batched ? draw : 0) * (a.x0_paths ? a.n_paths : 1) + (a.x0_paths ? path : 0)) * m + lane];
    obc_sim_put(xs, lane, x);
    bool hshort = false;
    for (int t = 0; t < n_steps; ++t) {
      // xu = T x (obc_sim_dot) + R eps_t (ascending c); lane c fetches eps_t[c] ahead of the product on T (k <= m <= 64)
      const bool shocked = t < nsh;
      const double e = shocked && lane < k ? eg[(size_t)t * k + lane] : 0.0;
      double xu = on ? obc_sim_dot(Tm + lane * ldm, xs, m) : 0.0;
      if (shocked) {  // (wave-uniform: readlane needs every lane)
        if (a.r_lds) {
          for (int c = 0; c < k; ++c) xu = fma(Rm[li * ldr + c], readlane_dyn_f64(e, c), xu);
        } else {
          for (int c = 0; c < k; ++c) xu = fma(rg[c], readlane_dyn_f64(e, c), xu);
        }
        xu = on ? xu : 0.0;
      }
      obc_sim_put(us, lane, xu);
      // q_h = c'T^h xu - bound (obc_sim_dot)
      double q = 1.0;
      if (act) {
        q = obc_sim_dot(Cq + lane * ldm, us, m) - bnd;
      }
      double nu = 0.0;
      int iters = 0;
      unsigned long long S;
      const int now = obc_regime_iterate<HM>(Mz, ldh, nub, lane, act, q, thr, max_iter, nu, iters, S);
      if (now != 0) {  // (wave-uniform)
        st = now;
        fail = t;
        fail_iters = iters;
        break;
      }
      hshort = hshort || ((S >> (H - 1)) & 1ull);
      // x = xu + W nu: the columns of S, ascending
      x = xu;
      if (on)
        for (unsigned long long bits = S; bits != 0ull; bits &= bits - 1ull) {
          const int j = __builtin_ctzll(bits);
          x = fma(W[lane * ldh + j], nub[j], x);
        }
      obc_sim_put(xs, lane, x);
      if (a.x_out && on) a.x_out[(row0 + t) * m + lane] = x;
      if (a.obs_out && lane < p) {
        double acc = 0.0;
        for (int i = 0; i < m; ++i) acc = fma(zg[i], xs[i], acc);
        a.obs_out[(row0 + t) * p + lane] = acc + dv;
      }
      if (a.plan_out && act) a.plan_out[(row0 + t) * H + lane] = nu;
      if (a.gap_out) {
        const double gp = wave_sum_dpp(ci * x) - bnd;
        if (lane == 0) a.gap_out[row0 + t] = gp;
      }
      if (lane == 0) {
        if (a.shadow_out) a.shadow_out[row0 + t] = nu;
        if (a.duration_out) a.duration_out[row0 + t] = __builtin_popcountll(S);
        if (a.iters_out) a.iters_out[row0 + t] = iters;
      }
    }
    if (hshort) st |= OBC_HORIZON_SHORT;
  }
  if (fail >= 0) {  // NaN from the period of the failure on
    const size_t f = row0 + fail, left = (size_t)(n_steps - fail);
    if (a.x_out) ps_fill_nan(a.x_out + f * m, left * m, lane, 64);
    if (a.obs_out) ps_fill_nan(a.obs_out + f * p, left * p, lane, 64);
    if (a.plan_out) ps_fill_nan(a.plan_out + f * H, left * H, lane, 64);
    if (a.gap_out) ps_fill_nan(a.gap_out + f, left, lane, 64);
    if (a.shadow_out) ps_fill_nan(a.shadow_out + f, left, lane, 64);
    for (size_t i = lane; i < left; i += 64) {
      if (a.duration_out) a.duration_out[f + i] = -1;
      if (a.iters_out) a.iters_out[f + i] = i == 0 ? fail_iters : 0;
    }
  }
  if (lane == 0) {
    a.pstat[pi] = st;
    if (a.pstat_out) a.pstat_out[pi] = st;
    if (a.fail_out) a.fail_out[pi] = fail;
  }
}

// the draw's word from its paths' bits (after obc_sim_kernel: another launch)
__global__ __launch_bounds__(OBC_THREADS) void obc_sim_status_kernel(int32_t* status, const int32_t* pstat, int batch, int n_paths) {
  const int draw = blockIdx.x * OBC_THREADS + threadIdx.x;
  if (draw >= batch) return;
  int any = 0;
  for (int j = 0; j < n_paths; ++j) any |= pstat[(size_t)draw * n_paths + j] & (OBC_NO_REGIME | OBC_SINGULAR);
  if (any) status[draw] |= OBC_ST_UNRESOLVED;
}

}  // namespace dsge
