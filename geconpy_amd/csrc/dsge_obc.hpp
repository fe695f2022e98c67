// OCCASIONALLY BINDING BOUND per draw: perfect-foresight paths of the linearised model (dsge_anticipated.hpp) on which c'x_t may not
// fall below a bound in the periods t < H.  The bound is enforced by anticipated "shadow" shocks nu_0 .. nu_{H-1} >= 0 on ONE shock
// column s (Holden and Paetz):
//     x_t = T x_{t-1} + w_t,   w_t = G w_{t+1} + R (e_t + nu_t e_s),   gap_t = c'x_t - bound,
//     gap_h >= 0,  nu_h >= 0,  nu_h gap_h = 0   for h < H.
// With Mz[h][j] = c'x_h of the path from x0 = 0 with a unit shock on column s at period j alone, and q_h = c'xu_h - bound on the
// unconstrained path xu: gap = q + Mz nu on h < H, a linear complementarity problem per path.  The REGIME ITERATION solves it:
//     S = {h : q_h < 0};  repeat:  nu = 0 off S,  Mz[S,S] nu_S = -q_S,  gap = q + Mz nu,
//     S' = {h in S : nu_h > 0} u {h not in S : gap_h < 0};  stop when S' == S (every comparison strict, no tolerance).
// The setup, the H unit-shock paths that give Mz, the unconstrained paths and the final paths on e' = e + nu e_s are the kernels of
// dsge_anticipated.hpp as they are (launch_obc.hip).  This file adds
//   obc_unit_kernel    the H unit-shock paths' shocks;
//   obc_regime_kernel  one wavefront per (draw, path), the four wavefronts of a workgroup on paths of ONE draw, whose Mz is staged
//                      once in the LDS ([H][H + 1], 32.5 KB at H = 64).  Lane h owns row h: q from the unconstrained path, then per
//                      iteration the rows of K = Mz[S,S] (a row off S, and a column off S, is not touched) in registers,
//                      Gauss-Jordan with row pivoting and NO row exchange -- pivot by the wave maximum of dsge_device.hpp (the lowest
//                      row among equal maxima), the pivot row through readlane_dyn_f64 -- S a 64-bit ballot, the fixed-point test a
//                      comparison of two scalars (the iteration itself: obc_regime_iterate of dsge_obc_regime.hpp, which the
//                      simulation kernel of dsge_obc_sim.hpp calls once per period).  A pivot with |pivot| <= rank_tol max|Mz| (or not finite), or a q_h that is not
//                      finite -> OBC_SINGULAR; max_iter solves without a fixed point -> OBC_NO_REGIME.  Writes nu, iters, the path's
//                      bits, max|q| and e' (zero rows up to max(n_shock_steps, H));
//   obc_gap_kernel     one wavefront per (draw, path): gap_t = c'x_t - bound on the final path, OBC_BEYOND_HORIZON when
//                      gap_t < -1e-12 max|q| at some t >= H, NaN over every output of a failed path, and the draw's status bit.
// No atomics: two calls give the same bits.
#pragma once
#include "dsge_obc_regime.hpp"

namespace dsge {

constexpr double OBC_BEYOND_TOL = 1e-12;

__host__ __device__ inline int obc_ld(int H) { return H + 1; }
// Mz [H][H + 1] and nu of every wavefront
__host__ __device__ inline size_t obc_lds_doubles(int H) { return (size_t)H * obc_ld(H) + OBC_WAVES * 64; }

struct ObcArgs {
  const double* mzt;     // [batch][H][H]: Mz[h][j] at j H + h (observation h of unit path j)
  const double* xu;      // [batch][n_paths][H][m]: the unconstrained paths, periods < H
  const double* x;       // [batch][n_paths][n_steps][m]: the final paths (gap kernel), or nullptr
  const double* c_row;   // [batch | 1][m]
  const double* bound;   // [batch | 1]
  const double* eps;     // [batch | 1][n_paths][n_shock_steps][k], or nullptr with n_shock_steps == 0
  int32_t* status;       // [batch] in/out or nullptr
  const int32_t* flag;   // [batch]: non-zero = M singular
  double* eps2;          // [batch][n_paths][nsp][k], nsp = max(n_shock_steps, H)
  double* qmax;          // [batch][n_paths]
  int32_t* pstat;        // [batch][n_paths]: the bits of the regime kernel
  double* nu_out;        // [batch][n_paths][H] or nullptr
  double* Mz_out;        // [batch][H][H] or nullptr
  int32_t* iters_out;    // [batch][n_paths] or nullptr
  int32_t* pstat_out;    // [batch][n_paths] or nullptr
  double* gap_out;       // [batch][n_paths][n_steps] or nullptr
  double* x_out;         // the caller's, each [batch][n_paths][n_steps][m | p] or nullptr
  double* w_out;
  double* obs_out;
  long long eps_draw;
  double rank_tol;
  int batch, m, k, p, n_paths, n_steps, n_shock_steps, nsp, H, shock, max_iter, c_batched, b_batched, groups;
};

// the shocks of the H unit paths: u[j][t][c] = 1 at t == j, c == s
__global__ __launch_bounds__(OBC_THREADS) void obc_unit_kernel(double* u, int H, int k, int s) {
  const int idx = blockIdx.x * OBC_THREADS + threadIdx.x;
  if (idx >= H * H * k) return;
  const int c = idx % k, t = idx / k % H, j = idx / (k * H);
  u[idx] = t == j && c == s ? 1.0 : 0.0;
}

// HM: 32 or 64, the rows of K a lane holds (obc_regime_iterate, dsge_obc_regime.hpp)
template <int HM>
__global__ __launch_bounds__(OBC_THREADS) void obc_regime_kernel(ObcArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, H = a.H, m = a.m, k = a.k;
  const int draw = blockIdx.x / a.groups, g = blockIdx.x - draw * a.groups;
  if (draw >= a.batch) return;
  const int path = g * OBC_WAVES + wv, ld = obc_ld(H);
  ks_lds* Mz = (ks_lds*)smem;              // [H][ld]
  ks_lds* nub = Mz + H * ld + wv * 64;     // [64]: nu of this wavefront's path
  const double* mg = a.mzt + (size_t)draw * H * H;
  for (int idx = tid; idx < H * H; idx += OBC_THREADS) {
    const int j = idx / H, h = idx - j * H;
    Mz[h * ld + j] = mg[idx];
  }
  __syncthreads();
  if (a.Mz_out && g == 0) {  // (NaN for a draw that was skipped: the unit paths' kernel has filled it)
    double* mo = a.Mz_out + (size_t)draw * H * H;
    for (int idx = tid; idx < H * H; idx += OBC_THREADS) {
      const int h = idx / H, j = idx - h * H;
      mo[idx] = Mz[h * ld + j];
    }
  }
  if (path >= a.n_paths) return;  // (no barrier below)
  const size_t pi = (size_t)draw * a.n_paths + path;
  const bool act = lane < H;
  int st = 0, iters = 0;
  double nu = 0.0, qm = 0.0;
  if ((a.status && a.status[draw] != 0) || a.flag[draw] != 0) {
    st = OBC_SKIPPED;
  } else {
    // q_h = c'xu_h - bound, ascending i
    const double* cr = ps_obs_slice(a.c_row, a.c_batched, draw, m);
    const double bnd = a.bound[a.b_batched ? draw : 0];
    double q = 1.0;
    if (act) {
      const double* xr = a.xu + (pi * H + lane) * m;
      double acc = 0.0;
      for (int i = 0; i < m; ++i) acc = fma(cr[i], xr[i], acc);
      q = acc - bnd;
    }
    double mmax = 0.0;
    if (act)
      for (int c = 0; c < H; ++c) mmax = fmax(mmax, fabs(Mz[lane * ld + c]));
    qm = act ? fabs(q) : 0.0;
    for (int off = 32; off >= 1; off >>= 1) {
      mmax = fmax(mmax, __shfl_xor(mmax, off));
      qm = fmax(qm, __shfl_xor(qm, off));
    }
    const double thr = (a.rank_tol > 0.0 ? a.rank_tol : 1e-14) * mmax;
    const int max_iter = a.max_iter > 0 ? a.max_iter : 64;
    unsigned long long S;
    st = obc_regime_iterate<HM>(Mz, ld, nub, lane, act, q, thr, max_iter, nu, iters, S);
  }
  const bool failed = st != 0;
  if (lane == 0) {
    a.pstat[pi] = st;
    a.qmax[pi] = qm;
    if (a.iters_out) a.iters_out[pi] = iters;
  }
  if (a.nu_out && act) a.nu_out[pi * H + lane] = failed ? NAN : nu;
  if (st == OBC_SKIPPED) return;  // (the final paths' kernel fills the draw with NaN and reads no shocks)
  // e' = e + nu e_s, zero rows beyond the caller's shocks
  __builtin_amdgcn_wave_barrier();
  nub[lane] = failed ? 0.0 : nu;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int nsh = a.n_shock_steps, nsp = a.nsp;
  const double* eg = nsh > 0 ? a.eps + (size_t)draw * a.eps_draw + (size_t)path * nsh * k : nullptr;
  double* e2 = a.eps2 + pi * nsp * k;
  for (int idx = lane; idx < nsp * k; idx += 64) {
    const int t = idx / k, c = idx - t * k;
    double v = t < nsh ? eg[idx] : 0.0;
    if (c == a.shock && t < H) v += nub[t];
    e2[idx] = v;
  }
}

__global__ __launch_bounds__(OBC_THREADS) void obc_gap_kernel(ObcArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, H = a.H, m = a.m, n_steps = a.n_steps;
  const int draw = blockIdx.x / a.groups, g = blockIdx.x - draw * a.groups;
  if (draw >= a.batch) return;
  const int path = g * OBC_WAVES + wv;
  if (path < a.n_paths) {
    const size_t pi = (size_t)draw * a.n_paths + path;
    int st = a.pstat[pi];
    if (st & OBC_FAILED) {
      if (a.x_out) ps_fill_nan(a.x_out + pi * n_steps * m, (size_t)n_steps * m, lane, 64);
      if (a.w_out) ps_fill_nan(a.w_out + pi * n_steps * m, (size_t)n_steps * m, lane, 64);
      if (a.obs_out) ps_fill_nan(a.obs_out + pi * n_steps * a.p, (size_t)n_steps * a.p, lane, 64);
      if (a.gap_out) ps_fill_nan(a.gap_out + pi * n_steps, (size_t)n_steps, lane, 64);
    } else if (a.x) {
      const double* cr = ps_obs_slice(a.c_row, a.c_batched, draw, m);
      const double bnd = a.bound[a.b_batched ? draw : 0], low = -OBC_BEYOND_TOL * a.qmax[pi];
      bool beyond = false;
      for (int t = lane; t < n_steps; t += 64) {
        const double* xr = a.x + (pi * n_steps + t) * m;
        double acc = 0.0;
        for (int i = 0; i < m; ++i) acc = fma(cr[i], xr[i], acc);
        const double gp = acc - bnd;
        if (a.gap_out) a.gap_out[pi * n_steps + t] = gp;
        beyond = beyond || (t >= H && gp < low);
      }
      if (__ballot(beyond) != 0ull) st |= OBC_BEYOND;
    }
    if (a.pstat_out && lane == 0) a.pstat_out[pi] = st;
  }
  // the draw's word, by the first workgroup of the draw (pstat is only read here)
  if (g == 0 && a.status) {
    int any = 0;
    for (int j = tid; j < a.n_paths; j += OBC_THREADS) any |= a.pstat[(size_t)draw * a.n_paths + j] & (OBC_NO_REGIME | OBC_SINGULAR);
    any = __syncthreads_or(any);
    if (any && tid == 0) a.status[draw] |= OBC_ST_UNRESOLVED;
  }
}

}  // namespace dsge
