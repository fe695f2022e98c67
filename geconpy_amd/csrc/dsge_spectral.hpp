// Spectral densities and filtered autocovariances per draw (dsge_spectral_moments_batched; docs/design/spectral_moments.md).
//
//   H_n = Zm (I - z_n T)^-1 R,  z_n = exp(-i w_n),  w_n = 2 pi n / N,  n = 0 .. N/2
//   F_n = H_n Q H_n^H (+ diag(Hdiag))
//   acov[j] = (1/N) sum_n c_n g_n Re(F_n exp(i w_n j))
//
// Two kernels.  spectral_solve_kernel<NC>: one wavefront per (draw, frequency group); T, R, Q, Z are staged in LDS once, then the
// wavefront takes the frequencies g, g + groups, ... of its draw.  Per frequency lane r holds row r of the complex [I - z T | R]
// in registers (NC >= m + k complex entries); Gauss-Jordan elimination with partial pivoting never moves a row: the pivot lane of
// a column is the unused lane with the largest modulus, its row reaches the other lanes through v_readlane (scalar operands of the
// update), and the used lanes are updated too, so no back substitution is left.  X goes to LDS once, then Zm X, (Zm X) Q and F_n
// are formed there and F_n is stored to scratch (and F_n / 2 pi to the spectrum).  spectral_reduce_kernel: one workgroup per draw
// sums the stored F_n over n in ascending order with cosines and sines from an LDS table -- no atomics, and no dependence on the
// grouping above -- and writes the NaN and the status bit of a skipped or singular draw.
#pragma once
#include "dsge_postsolve.hpp"  // the per-draw slices of Q, Z, Hdiag and the NaN fill (docs/design/dynamics.md, "the shared pieces")

#include "../../include/dsge_hip.h"

namespace dsge {

constexpr int SP_REDUCE_THREADS = 256;
constexpr int SP_LAGS = 8;  // lags one pass of the reduction keeps in registers
constexpr int SP_BLK = 8;   // columns under one uniform branch of the elimination

struct SpectralArgs {
  const double *T, *R, *Q, *Z, *Hdiag, *gain;
  int q_mode, z_batched, h_batched;
  int batch, m, k, p, dim, n_grid, nf, n_lags, correlation, groups;
  int solve_all;  // the spectrum is wanted: frequencies of zero gain are solved too
  double rank_tol;
  const int32_t* status_in;
  int32_t* status;
  int32_t* flag;   // scratch [batch]: set by the solve kernel when a pivot fails
  double2* F;      // scratch [batch][nf][dim][dim], null when acov is null
  double* acov;    // [batch][n_lags + 1][dim][dim] or null
  double2* spec;   // [batch][nf][dim][dim] or null
};

// the real part of the solve kernel's LDS image, in doubles (even): T [m][m|1], R [m][k|1], Q [k][k], Z [p][m], Hdiag [p]
__host__ __device__ inline size_t sp_real_doubles(int m, int k, int p, int has_z) {
  const size_t real = (size_t)m * (m | 1) + (size_t)m * (k | 1) + (size_t)k * k + (has_z ? (size_t)p * m + p : 0);
  return (real + 1) & ~(size_t)1;
}
// doubles of the solve kernel's LDS image: the real part, then complex X [m][k|1], (Z: H [p][k|1],) G [dim][k|1]
__host__ __device__ inline size_t sp_solve_lds_doubles(int m, int k, int p, int has_z) {
  const int dim = has_z ? p : m;
  return sp_real_doubles(m, k, p, has_z) + 2 * (size_t)(m + dim + (has_z ? p : 0)) * (k | 1);
}
__host__ __device__ inline size_t sp_reduce_lds_doubles(int n_grid, int dim) { return 2 * (size_t)n_grid + dim; }

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(fma(a.x, b.x, -a.y * b.y), fma(a.x, b.y, a.y * b.x));
}
// a - l b
__device__ __forceinline__ double2 cfnma(double2 l, double2 b, double2 a) {
  a.x = fma(-l.x, b.x, a.x); a.x = fma(l.y, b.y, a.x);
  a.y = fma(-l.x, b.y, a.y); a.y = fma(-l.y, b.x, a.y);
  return a;
}
// 1 / a
__device__ __forceinline__ double2 cinv(double2 a) {
  const double s = 1.0 / fma(a.x, a.x, a.y * a.y);
  return make_double2(a.x * s, -a.y * s);
}
// the value lane `src` (uniform) holds
__device__ __forceinline__ double readlane_f64(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// max(v, the value of the lane the DPP control names); a lane without a source keeps its own
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_max_u64(unsigned long long v) {
  const int lo = (int)v, hi = (int)(v >> 32);
  const int olo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  const int ohi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  const unsigned long long o = ((unsigned long long)(unsigned)ohi << 32) | (unsigned)olo;
  return o > v ? o : v;
}

// The row lives in registers only because the two empty asm statements below steer the allocation (NC = 96: 256 VGPRs + 189 AGPRs).
// After a compiler update compile launch_spectral.hip with -Rpass-analysis=kernel-resource-usage and read "ScratchSize [bytes/lane]"
// of every instance: it must be 0 (tests/test_spectral_moments_frontend.py does exactly that).
template <int NC>
__global__ __launch_bounds__(64) void spectral_solve_kernel(SpectralArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x, m = a.m, k = a.k, p = a.p, dim = a.dim, ldt = m | 1, ldr = k | 1, ldh = k | 1, ncol = m + k;
  const int draw = blockIdx.x / a.groups, grp = blockIdx.x - draw * a.groups;
  if (a.status_in && a.status_in[draw] != 0) return;
  const bool has_z = a.Z != nullptr;
  double* Ts = smem;
  double* Rs = Ts + m * ldt;
  double* Qs = Rs + m * ldr;
  double* Zs = Qs + k * k;
  double* Hd = Zs + (has_z ? p * m : 0);
  double2* Xs = reinterpret_cast<double2*>(smem + sp_real_doubles(m, k, p, has_z));  // [m][ldh]    X = (I - z T)^-1 R
  double2* Hc = has_z ? Xs + (size_t)m * ldh : Xs;                                   // [dim][ldh]  Zm X
  double2* Gc = Hc + (size_t)dim * ldh;                                              // [dim][ldh]  (Zm X) Q

  // ---- stage the draw
  const double* Tg = a.T + (size_t)draw * m * m;
  const double* Rg = a.R + (size_t)draw * m * k;
  for (int i = lane; i < m * m; i += 64) Ts[(i / m) * ldt + i % m] = Tg[i];
  for (int i = lane; i < m * k; i += 64) Rs[(i / k) * ldr + i % k] = Rg[i];
  {
    const bool qd = a.q_mode == DSGE_Q_DIAG_SHARED || a.q_mode == DSGE_Q_DIAG_BATCHED;
    const bool qb = a.q_mode == DSGE_Q_DIAG_BATCHED || a.q_mode == DSGE_Q_FULL_BATCHED;
    const double* Qg = a.Q + (qb ? (size_t)draw * (qd ? k : k * k) : 0);
    for (int i = lane; i < k * k; i += 64) {
      const int r = i / k, c = i - r * k;
      Qs[i] = qd ? (r == c ? Qg[r] : 0.0) : Qg[i];
    }
  }
  if (has_z) {
    const double* Zg = a.Z + (a.z_batched ? (size_t)draw * p * m : 0);
    for (int i = lane; i < p * m; i += 64) Zs[i] = Zg[i];
    for (int i = lane; i < p; i += 64) Hd[i] = a.Hdiag ? ps_obs_slice(a.Hdiag, a.h_batched, draw, p)[i] : 0.0;
  }
  const double tol = a.rank_tol > 0.0 ? a.rank_tol : 1e-12;
  const double inv_2pi = 0.15915494309189535;
  const bool live = lane < m;  // lane r holds row r
  const int lr = live ? lane : 0;
  wave_sync();

  for (int n = grp; n < a.nf; n += a.groups) {
    if (!a.solve_all && a.gain && a.gain[n] == 0.0) continue;  // uniform: not solved, not read by the reduction
    double sn, cs;
    sincospi(2.0 * (double)n / (double)a.n_grid, &sn, &cs);
    if (n == 0) { cs = 1.0; sn = 0.0; }
    if (2 * n == a.n_grid) { cs = -1.0; sn = 0.0; }
    const double zr = cs, zi = -sn;  // z = exp(-i w)
    // ---- row `lane` of the pencil [I - z T | R]; max |entry|^2 of the left part
    double2 row[NC];
    double amax2 = 0.0;
    int lo = lane, mo = m;  // opaque per frequency: the comparisons below stay inside the loop instead of living in registers
    asm volatile("" : "+v"(lo), "+s"(mo));
#pragma unroll
    for (int cb = 0; cb < NC / SP_BLK; ++cb) {
#pragma unroll
      for (int u = 0; u < SP_BLK; ++u) {
        const int c = cb * SP_BLK + u;
        double2 v = make_double2(0.0, 0.0);
        if (c < mo) {
          const double t = live ? Ts[lr * ldt + c] : 0.0;
          v = make_double2((lo == c ? 1.0 : 0.0) - zr * t, -zi * t);
          amax2 = nanmax(amax2, fma(v.x, v.x, v.y * v.y));
        } else if (c < mo + k) {
          v = make_double2(live ? Rs[lr * ldr + (c - mo)] : 0.0, 0.0);
        }
        row[c] = v;
      }
      asm volatile("" ::: "memory");  // at most SP_BLK loads in flight: the row, not the loads, sets the register count
    }
    amax2 = wave_nanmax(amax2);
    const double thr2 = tol * tol * amax2;
    bool singular = !(amax2 == amax2);
    // ---- Gauss-Jordan elimination with partial pivoting over the unused lanes
    bool used = !live;
    int my_col = 0;
    double2 my_pv = make_double2(1.0, 0.0);
    for (int j = 0; j < m && !singular; ++j) {
      double2 lj = make_double2(0.0, 0.0);  // row[j]
#pragma unroll
      for (int cb = 0; cb < NC / SP_BLK; ++cb)
        if ((j / SP_BLK) == cb) {
#pragma unroll
          for (int u = 0; u < SP_BLK; ++u)
            if ((j % SP_BLK) == u) lj = row[cb * SP_BLK + u];
        }
      // one 64-bit key per lane: the bits of |.|^2 (non-negative: ordered as integers) with the low 6 bits replaced by 63 - lane
      const double v2 = fma(lj.x, lj.x, lj.y * lj.y);
      unsigned long long key = used ? 0ull : (((unsigned long long)__double_as_longlong(v2) & ~63ull) | (unsigned)(63 - lane));
      // prefix maxima along the 16-lane rows, then across them: lane 63 ends with the maximum of the wavefront
      key = dpp_max_u64<0x111>(key);  // row_shr:1
      key = dpp_max_u64<0x112>(key);  // row_shr:2
      key = dpp_max_u64<0x114>(key);  // row_shr:4
      key = dpp_max_u64<0x118>(key);  // row_shr:8
      key = dpp_max_u64<0x142>(key);  // row_bcast:15
      key = dpp_max_u64<0x143>(key);  // row_bcast:31
      key = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(key >> 32), 63) << 32) |
            (unsigned)__builtin_amdgcn_readlane((int)key, 63);
      const int piv = 63 - (int)(key & 63ull);
      const double best = __longlong_as_double((long long)(key & ~63ull));
      if (!(best > thr2) || piv >= m) { singular = true; break; }  // (uniform; a NaN fails the comparison)
      const double2 pv = make_double2(readlane_f64(lj.x, piv), readlane_f64(lj.y, piv));
      const bool mine = lane == piv;
      const double2 l = mine ? make_double2(0.0, 0.0) : cmul(lj, cinv(pv));
      if (mine) { used = true; my_col = j; my_pv = lj; }
#pragma unroll
      for (int cb = 0; cb < NC / SP_BLK; ++cb)
        if (cb * SP_BLK + SP_BLK - 1 > j && cb * SP_BLK < ncol) {  // uniform; a column <= j is dead: updating it is harmless
#pragma unroll
          for (int u = 0; u < SP_BLK; ++u) {
            const int c = cb * SP_BLK + u;
            const double2 pj = make_double2(readlane_f64(row[c].x, piv), readlane_f64(row[c].y, piv));
            row[c] = cfnma(l, pj, row[c]);
          }
        }
    }
    if (singular) {  // uniform over the wavefront
      if (lane == 0) a.flag[draw] = 1;
      return;
    }
    // ---- X: the lane that was the pivot of column j holds x_j times its pivot
    {
      const double2 ip = cinv(my_pv);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c >= m && c < ncol && live) Xs[my_col * ldh + (c - m)] = cmul(row[c], ip);
    }
    wave_sync();
    // ---- H = Zm X (Z == NULL: H is X)
    if (has_z) {
      for (int e = lane; e < dim * k; e += 64) {
        const int r = e / k, c = e - r * k;
        double2 h = make_double2(0.0, 0.0);
        for (int i = 0; i < m; ++i) {
          const double z = Zs[r * m + i];
          const double2 x = Xs[i * ldh + c];
          h.x = fma(z, x.x, h.x);
          h.y = fma(z, x.y, h.y);
        }
        Hc[r * ldh + c] = h;
      }
      wave_sync();
    }
    // ---- G = H Q
    for (int e = lane; e < dim * k; e += 64) {
      const int r = e / k, c = e - r * k;
      double2 g = make_double2(0.0, 0.0);
      for (int i = 0; i < k; ++i) {
        const double q = Qs[i * k + c];
        const double2 h = Hc[r * ldh + i];
        g.x = fma(h.x, q, g.x);
        g.y = fma(h.y, q, g.y);
      }
      Gc[r * ldh + c] = g;
    }
    wave_sync();
    // ---- F = G H^H (+ diag(Hdiag))
    double2* Fo = a.F + ((size_t)draw * a.nf + n) * dim * dim;
    double2* So = a.spec ? a.spec + ((size_t)draw * a.nf + n) * dim * dim : nullptr;
    for (int e = lane; e < dim * dim; e += 64) {
      const int r = e / dim, c = e - r * dim;
      double2 f = make_double2(0.0, 0.0);
      for (int i = 0; i < k; ++i) {
        const double2 g = Gc[r * ldh + i], h = Hc[c * ldh + i];  // g conj(h)
        f.x = fma(g.x, h.x, f.x); f.x = fma(g.y, h.y, f.x);
        f.y = fma(g.y, h.x, f.y); f.y = fma(-g.x, h.y, f.y);
      }
      if (has_z && r == c) f.x += Hd[r];
      if (a.F) Fo[e] = f;
      if (So) So[e] = make_double2(f.x * inv_2pi, f.y * inv_2pi);
    }
    wave_sync();
  }
}

// sum over n, ascending, of w_n Re(F_n[e] exp(i w_n j)) for the lags j0 .. j0 + SP_LAGS - 1
__device__ __forceinline__ void sp_accumulate(const SpectralArgs& a, const double2* __restrict__ Fd, const double* ct, const double* st,
                                              int e, int j0, double (&acc)[SP_LAGS]) {
  const int N = a.n_grid, dd = a.dim * a.dim;
  const double inv_n = 1.0 / (double)N;
#pragma unroll
  for (int u = 0; u < SP_LAGS; ++u) acc[u] = 0.0;
  for (int n = 0; n < a.nf; ++n) {
    const double g = a.gain ? a.gain[n] : 1.0;
    if (a.gain && g == 0.0) continue;
    const double w = ((n == 0 || 2 * n == N) ? 1.0 : 2.0) * g * inv_n;
    const double2 f = Fd[(size_t)n * dd + e];
    int idx = (int)(((long long)n * j0) % N);
#pragma unroll
    for (int u = 0; u < SP_LAGS; ++u) {
      const double t = fma(f.x, ct[idx], -f.y * st[idx]);
      acc[u] = fma(w, t, acc[u]);
      idx += n;
      if (idx >= N) idx -= N;
    }
  }
}

__global__ __launch_bounds__(SP_REDUCE_THREADS) void spectral_reduce_kernel(SpectralArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x, draw = blockIdx.x, dim = a.dim, dd = dim * dim, N = a.n_grid;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const bool skipped = a.status_in && a.status_in[draw] != 0;
  const bool singular = !skipped && a.flag[draw] != 0;
  if (skipped || singular) {
    if (a.acov) {
      double* o = a.acov + (size_t)draw * (a.n_lags + 1) * dd;
      for (size_t i = tid; i < (size_t)(a.n_lags + 1) * dd; i += SP_REDUCE_THREADS) o[i] = qnan;
    }
    if (a.spec) {
      double2* o = a.spec + (size_t)draw * a.nf * dd;
      for (size_t i = tid; i < (size_t)a.nf * dd; i += SP_REDUCE_THREADS) o[i] = make_double2(qnan, qnan);
    }
    if (singular && a.status && tid == 0) a.status[draw] |= DSGE_ST_SPECTRAL_SINGULAR;
    return;
  }
  if (!a.acov) return;
  double* ct = smem;      // cos(2 pi i / N)
  double* st = ct + N;    // sin(2 pi i / N)
  double* sd = st + N;    // 1 / std or 1
  for (int i = tid; i < N; i += SP_REDUCE_THREADS) {
    double s, c;
    sincospi(2.0 * (double)i / (double)N, &s, &c);
    if (i == 0) { c = 1.0; s = 0.0; }
    if (2 * i == N) { c = -1.0; s = 0.0; }
    ct[i] = c;
    st[i] = s;
  }
  __syncthreads();
  const double2* Fd = a.F + (size_t)draw * a.nf * dd;
  double acc[SP_LAGS];
  for (int r = tid; r < dim; r += SP_REDUCE_THREADS) {
    double s = 1.0;
    if (a.correlation) {
      sp_accumulate(a, Fd, ct, st, r * dim + r, 0, acc);  // the bits of acov[0][r][r]
      s = 1.0 / sqrt(acc[0]);
    }
    sd[r] = s;
  }
  __syncthreads();
  double* o = a.acov + (size_t)draw * (a.n_lags + 1) * dd;
  for (int e = tid; e < dd; e += SP_REDUCE_THREADS) {
    const int r = e / dim, c = e - r * dim;
    for (int j0 = 0; j0 <= a.n_lags; j0 += SP_LAGS) {
      sp_accumulate(a, Fd, ct, st, e, j0, acc);
#pragma unroll
      for (int u = 0; u < SP_LAGS; ++u)
        if (j0 + u <= a.n_lags) o[(size_t)(j0 + u) * dd + e] = acc[u] * sd[r] * sd[c];
    }
  }
}

}  // namespace dsge
